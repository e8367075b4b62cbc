"""The last level's cat-mix adjoint inside its CG adjoint launch (backward.inc: k_catbuild_bwd_mfma<false, false, true>).

At small mini-batches on the one-launch-per-level path the waves of the last level's CG adjoint form their slice of the
concatenated-channel adjoint themselves -- d_cat = dA_next W^H on the matrix cores, from the atom's rows of dA_next and the packed
weights Lin::mx that the weight preparation derives -- instead of loading what k_gemm_mfma_cols_ws stored.  MG_CGB_FUSED_MIX = 1 / 0
(read at every step) forces the form on / off; every case below runs both and holds both to the float64 oracle.

Shapes, canvas 7 and 9 at zs = [0, 9, 16], six samples:
  c7   0, 1, 2, 7, 3, 6 atoms: no item; the own atom as the only neighbour; one neighbour; a full tile minus one; 19 atoms, so the
       (atom, channel) items are no multiple of the four wave slots of a workgroup wherever CH allows it (CH = 8 cannot) and the
       last persistent round is partial
  c9   0, 1, 2, 7, 8, 9 atoms: a full neighbour tile, and a second tile of one neighbour; 27 atoms
Builds: the default (10, 4) at 3 levels, the channel variants (8, 2), (7, 3), (9, 5), (1, 1) and num_cg_levels = 2 / 4.  The last
level's cat-mix has 2 Co = 2 Z CE real outputs: 24 in the default build (all six k steps of the product), 12 / 18 / 6 in three
variants (k steps that are zero or partial), 30 at CE = 5 -- more than the instance holds.  Which builds take the instance is pinned
(_fuses): (9, 5) keeps the column GEMM whatever the switch says, and so do num_cg_levels = 2 / 4, whose steps never take the
one-launch-per-level path (level0.inc: NLEV == 3); for those three the test holds the launches of both switch settings equal.

Bounds are the project's own (tests/helpers.py): gradients assert_grads' defaults; outputs (where a test holds them: the forward is
not what changes here) rel_err < 1e-5.  The saved adjoints d_Elast_l and d_A{last}_l are gradients with respect to intermediates
and are held to the oracle like the gradients are, 2e-4 of their maximum (assert_grads' first bound), not to the 1e-5 of a saved
forward stage: the UNFUSED form, which is the parent commit's code, measures 1.014e-5 on d_Elast_0 of (10, 4, 3) at c7 (the fused
form 1.016e-5) and 7.4e-6 or less in every other case, and 2.434e-5 on d_A2_0 (fused 2.437e-5), 7.1e-6 or less elsewhere, so 1e-5
is not a bound float32 keeps there with either form.  The two forms
against each other are held to 1e-5 of the maximum (measured: 5.5e-7 at most) -- they differ by the summation order inside a
slice and by float atomics only."""
import numpy as np
import pytest
import torch

from molgym_amd.synthetic import CONFIGS
from tests.helpers import PPO_HP as HP, assert_grads, compact_edges, compact_vec, crowded, device_batch, grad_report, launch_log, make_pair, rel_err

pytestmark = pytest.mark.gpu
SWITCH = 'MG_CGB_FUSED_MIX'
FUSED = 'k_catbuild_bwd_mfma<false, false, true>'
SHAPES = {'c7': (7, [0, 1, 2, 7, 3, 6]), 'c9': (9, [0, 1, 2, 7, 8, 9])}
BUILDS = [(10, 4, 3), (8, 2, 3), (7, 3, 3), (9, 5, 3), (1, 1, 3), (10, 4, 2), (10, 4, 4)]
CASES = [(b, s) for b in BUILDS for s in SHAPES]
_bid = lambda b: 'c%de%dl%d' % b
# which builds take the fused instance on these shapes: 2 Z CE real outputs within the 4 CGX_KS the instance multiplies (cg_mfma.inc),
# and the one-launch-per-level path, which exists at three levels only (level0.inc)
_fuses = lambda b: 2 * 3 * b[1] <= 24 and b[2] == 3
_ids = lambda v: _bid(v[0]) + '-' + v[1]


@pytest.fixture(autouse=True)
def _restore_switches(built_lib):
    from molgym_amd import _lib
    prev = (_lib.is_deterministic(), _lib.is_deterministic_covariant())
    yield
    _lib.set_deterministic(prev[0], covariant=prev[1])


def _pair_data(build, shape, data_seed=0):
    canvas, counts = SHAPES[shape] if isinstance(shape, str) else shape
    name = f'cfg2_canvas{canvas}'
    CONFIGS.setdefault(name, dict(CONFIGS['cfg2'], canvas_size=canvas))
    ac, ref, cfg = make_pair(name, seed=500 + 10 * build[0] + canvas + build[2], num_channels_hidden=build[0],
                             num_channels_per_element=build[1], num_cg_levels=build[2])
    data = crowded(name, counts, 91 + canvas + data_seed)
    if not np.isfinite(data['adv']).all():
        data['adv'] = np.linspace(0.7, -0.4, len(data['adv']))
    return ac, ref, cfg, data


def _weights(B):
    g = torch.Generator().manual_seed(9)
    return tuple(torch.randn(B, generator=g, dtype=torch.float64) * s for s in (1.0, 0.3, 0.7))


def _step_backward(ac, data, w):
    ac.theta.grad = None
    out = ac.step(data['obs'], data['act'])
    (out['logp'].double() * w[0].cuda() + out['ent'].double() * w[1].cuda() + out['v'].double() * w[2].cuda()).sum().backward()
    torch.cuda.synchronize()
    return {k: out[k].detach().cpu() for k in ('logp', 'ent', 'v')}, ac.theta.grad.detach().cpu().clone()


def _oracle(ref, data, w):
    """outputs, the gradient of every parameter, the adjoint of the last edge level's mix (before the soft mask: what the CG
    adjoint of the last level stores, d_Elast) and the adjoint of the representations that enter the last level (d_A{last}) of the
    float64 oracle"""
    kept, kept_a = [], []
    cgm = ref.cg_model.cormorant_cg
    keep = lambda into: (lambda m, i, o: into.append([p for p in o if p.retain_grad() is None]))
    hooks = [cgm.edge_levels[-1].cat_mix.register_forward_hook(keep(kept)), cgm.atom_levels[-2].register_forward_hook(keep(kept_a))]
    try:
        ref.zero_grad()
        exp = ref.step(data['obs'], data['act'], dtype=torch.float64)
        (exp['logp'] * w[0] + exp['ent'] * w[1] + exp['v'] * w[2]).sum().backward()
    finally:
        for h in hooks:
            h.remove()
    assert len(kept) == 1 and len(kept_a) == 1
    want = {k: type('G', (), {'grad': (p.grad if p.grad is not None else torch.zeros_like(p)).detach().clone()})
            for k, p in ref.named_parameters()}
    return ({k: exp[k].detach() for k in ('logp', 'ent', 'v')}, want, [p.grad.detach().clone() for p in kept[0]],
            [p.grad.detach().clone() for p in kept_a[0]])


def _views(ac, cfg, data, levels):
    """what the last level's CG adjoint leaves behind it: the edge adjoints it stores, and the adjoint of the representations it
    reads after the edge level has folded the channel-major accumulator into it"""
    from oracle.covariant_ref import parse_observations
    d = parse_observations(data['obs'], cfg['zs'], cfg['canvas_size'], torch.float64)
    ccfg = ac._make_cfg(len(data['obs']), d['num_atoms'].numpy())
    names = [f'd_Elast_{l}' for l in range(5)] + [f'd_A{levels - 1}_{l}' for l in range(5)]
    return d, ccfg, {n: ac.workspace_view(n, ccfg).detach().cpu().clone() for n in names}


def _stage_err(got, want):
    return (got.double() - want.double()).abs().max().item() / max(want.abs().max().item(), 1e-30)


_RUNS = {}


@pytest.fixture(scope='module', autouse=True)
def _drop_runs():
    yield
    _RUNS.clear()   # agents, workspaces and oracle results of this module do not outlive it


def _run(build, shape, monkeypatch):
    """both forms of the product and the oracle, once per (build, shape); nothing here is changed afterwards"""
    key = (build, shape)
    if key not in _RUNS:
        ac, ref, cfg, data = _pair_data(build, shape)
        w = _weights(len(data['obs']))
        rec = dict(ac=ac, ref=ref, cfg=cfg, data=data, w=w)
        for form in ('1', '0'):
            monkeypatch.setenv(SWITCH, form)
            out, grad = _step_backward(ac, data, w)
            d, ccfg, views = _views(ac, cfg, data, build[2])
            rec[form] = dict(out=out, grad=grad, views=views)
        rec['d'], rec['ccfg'] = d, ccfg
        rec['exp'], rec['want'], rec['dE'], rec['dA'] = _oracle(ref, data, w)
        del rec['ref']   # (the float64 oracle is not needed again)
        _RUNS[key] = rec
    return _RUNS[key]


def _assert_one_launch_fewer(names, at, build):
    g = len(names['0']) - len(names['1'])   # the column GEMM of the level: one grouped launch, or one per degree in some builds
    gone = names['0'][at:at + g]
    print('launches that went away:', gone)
    assert g >= 1 and all('gemm' in n for n in gone) and 'k_catbuild_bwd_mfma<false>' in names['0'][at + g]
    assert names['1'][:at] == names['0'][:at] and names['1'][at + 1:] == names['0'][at + g + 1:]
    if build == (10, 4, 3):
        assert g == 1 and 'cols_ws' in gone[0]


def _ppo_log(ac, data):
    batch = device_batch(ac, data)
    ac.theta.grad = torch.zeros_like(ac.theta)
    with launch_log(ac._L()) as log:
        ac.ppo_minibatch(batch, *HP, graph=False)
    torch.cuda.synchronize()
    assert torch.isfinite(ac.theta.grad).all()
    return log


# ---- parity: every gradient slot, both forms ------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_every_gradient_slot_vs_oracle_in_both_forms(built_lib, monkeypatch, case):
    build, shape = case
    run = _run(build, shape, monkeypatch)
    for form in ('1', '0'):
        errs = {k: rel_err(run[form]['out'][k], run['exp'][k]) for k in ('logp', 'ent', 'v')}
        report = grad_report(run[form]['grad'].double(), run['want'], run['ac'].slot_table)
        print(f'build {build} shape {shape} {SWITCH}={form}: outputs {errs}; worst gradient slot (err / slot max)',
              max(v[0] for v in report.values() if v[1] >= 1e-10))
        assert bool(torch.isfinite(run[form]['grad']).all())
        assert_grads(report)
    for k in ('logp', 'ent', 'v'):   # (the forward is the same code in both)
        assert torch.equal(run['1']['out'][k], run['0']['out'][k]), k


# ---- the slice, without exposing LDS: what the kernel writes from it ------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_last_level_adjoints_of_both_forms_and_the_launch_log(built_lib, monkeypatch, case):
    """(i) the launch log of a one-call step: forced on, the fused instance ran ONCE (the last level) and the column GEMM of that
    level did not; forced off, the instance never ran.  The step has one launch fewer with it.  (ii) d_Elast_l, stored by the kernel
    from the rebuilt adjoint moments of the slice, of both forms against the oracle's adjoint of the last edge mix, and against
    each other; d_A{last}_l (the slice's power and aggregate products, folded by the edge level) of the two forms against each
    other."""
    build, shape = case
    run = _run(build, shape, monkeypatch)
    ac, data = run['ac'], run['data']
    names = {}
    fuses = _fuses(build)
    for form in ('0', '1'):
        monkeypatch.setenv(SWITCH, form)
        log = _ppo_log(ac, data)
        names[form] = list(log.names)
        if form == '0':   # the gate of the instance is the one-launch-per-level path: three-level builds take it on these shapes
            assert any('k_edge_bwd' in n for n in log.names) == (build[2] == 3)
        n_fused = sum(1 for n in log.names if FUSED in n)
        print(f'build {build} shape {shape} {SWITCH}={form}: {len(log.names)} launches, fused {n_fused}')
        assert n_fused == (1 if form == '1' and fuses else 0)
        assert log.ran('k_catbuild_bwd_mfma<false>') == (form == '0' or build[2] > 2 or not fuses)   # (the levels below stay)
    # the same launches in the same order, but: the fused instance in the place of the last level's unfused one, and the launch in
    # front of it -- the column GEMM of that level's cat-mix adjoint -- gone
    if not fuses:
        assert names['1'] == names['0']
    at = next((j for j, n in enumerate(names['1']) if FUSED in n), None) if fuses else None
    if at is not None:
        _assert_one_launch_fewer(names, at, build)
    em = run['d']['edge_mask']
    want = compact_edges(run['dE'], em)
    want_a = compact_vec(run['dA'], run['d']['atom_mask'])
    for l in range(5):
        n = want[l].numel()
        a, b = run['1']['views'][f'd_Elast_{l}'][:n].view(want[l].shape), run['0']['views'][f'd_Elast_{l}'][:n].view(want[l].shape)
        ea, eb, eab = _stage_err(a, want[l]), _stage_err(b, want[l]), _stage_err(a, b)
        print(f'd_Elast_{l}: fused vs oracle {ea:.3e}, unfused vs oracle {eb:.3e}, fused vs unfused {eab:.3e}')
        assert ea < 2e-4 and eb < 2e-4 and eab < 1e-5, (l, ea, eb, eab)
        name = f'd_A{build[2] - 1}_{l}'
        n = want_a[l].numel()
        a, b = run['1']['views'][name][:n].view(want_a[l].shape), run['0']['views'][name][:n].view(want_a[l].shape)
        ea, eb, eab = _stage_err(a, want_a[l]), _stage_err(b, want_a[l]), _stage_err(a, b)
        print(f'{name}: fused vs oracle {ea:.3e}, unfused vs oracle {eb:.3e}, fused vs unfused {eab:.3e}')
        assert b.abs().max().item() > 0 and ea < 2e-4 and eb < 2e-4 and eab < 1e-5, (name, ea, eb, eab)


# ---- a second step on the same workspace ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('build', [(10, 4, 3), (7, 3, 3)], ids=_bid)
def test_second_step_on_the_same_workspace(built_lib, monkeypatch, build):
    """two sets of canvases of one shape through the same agent and workspace, the fused form on: the accumulators the kernel adds
    to are zeroed by the step itself (k_heads_bwd), the packed weights stay current.  The SECOND step is held to the oracle."""
    monkeypatch.setenv(SWITCH, '1')
    ac, ref, cfg, first = _pair_data(build, 'c7')
    second = crowded('cfg2_canvas7', SHAPES['c7'][1], 1091)
    w = _weights(len(second['obs']))
    _step_backward(ac, first, w)
    out, grad = _step_backward(ac, second, w)
    exp, want, _, _ = _oracle(ref, second, w)
    report = grad_report(grad.double(), want, ac.slot_table)
    print(f'build {build} second step: worst gradient slot (err / slot max)', max(v[0] for v in report.values() if v[1] >= 1e-10))
    for k in ('logp', 'ent', 'v'):
        assert rel_err(out[k], exp[k]) < 1e-5, k
    assert bool(torch.isfinite(grad).all())
    assert_grads(report)


# ---- shapes and modes that keep the two-launch form -----------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['canvas12', 'ordered'])
def test_fallback_shapes_keep_the_column_gemm(built_lib, monkeypatch, mode):
    """canvas 12 is past the one-launch-per-level path (edge_level.inc: N <= 9); ordered mode keeps every launch it had.  Forced
    on, neither runs the fused instance; both stay oracle-green."""
    import molgym_amd
    monkeypatch.setenv(SWITCH, '1')
    build = (10, 4, 3)
    shape = (12, [0, 1, 10, 12]) if mode == 'canvas12' else SHAPES['c7']
    ac, ref, cfg, data = _pair_data(build, shape)
    if mode == 'ordered':
        molgym_amd.set_deterministic(True, covariant=True)
    w = _weights(len(data['obs']))
    out, grad = _step_backward(ac, data, w)
    exp, want, _, _ = _oracle(ref, data, w)
    for k in ('logp', 'ent', 'v'):
        assert rel_err(out[k], exp[k]) < 1e-5, k
    assert_grads(grad_report(grad.double(), want, ac.slot_table))
    log = _ppo_log(ac, data)
    monkeypatch.setenv(SWITCH, '0')
    off = _ppo_log(ac, data)
    print(mode, sorted(set(log.names)))
    assert not any(FUSED in n for n in log.names)
    assert log.ran('k_catbuild_bwd_mfma<false, true>' if mode == 'ordered' else 'k_catbuild_bwd_mfma<false>')
    assert log.names == off.names   # (the switch changes nothing here: the column GEMM of the last level included)
