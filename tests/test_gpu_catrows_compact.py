"""The stored rows of the atom cat-mix of the levels >= 1 on the GPU: 35 of the 65 CG power blocks are kept, the weights folded.

The rows `cat_a{k}_{l}` (k >= 1) hold [ag | in | kept sq] per channel (tests/test_catrow_map_host.py pins the map and the rule behind
it to the oracle); the derived weights of the mix carry W[kept part] + s W[mirrored part]; k_fold_weights hands the entry of the
derived gradient to both parts.  theta, its gradient and the parameter layout keep the reference's shape.

Shapes (the smallest at which each path can go wrong):
  c7    canvas 7, four samples with 0, 1, 2 and 7 atoms: no item, no neighbour, one neighbour, a partial neighbour tile
  c12   canvas 12, two samples with 10 and 12 atoms: a second neighbour tile
Builds: the default (10, 4) and the odd (7, 3), where K = 14 W' is no multiple of 4 and the epilogue of k_edge_bwd_mix gives way to
the column GEMM.

Bounds are the project's own (tests/helpers.py): gradients assert_grads (2e-4 of the slot maximum, 1e-2 relative on the entries above
1 % of it); a saved intermediate max |err| / max |want| < 1e-5, the bound encoder_stage_report's callers hold every other saved
stage of the encoder to (a row entry is a sum of up to ~100 float32 products of O(1) factors with cancellation, so an elementwise
relative bound is not one float32 can keep)."""
import ctypes as C

import numpy as np
import pytest
import torch

from molgym_amd.synthetic import CONFIGS
from oracle import so3
from tests.helpers import PPO_HP as HP, assert_grads, crowded, device_batch, grad_report, make_pair, oracle_backward
from tests.test_catrow_map_host import NBLK, WIDTHS, expected_map

pytestmark = pytest.mark.gpu
BUILDS = [(10, 4), (7, 3)]
SHAPES = {'c7': (7, [0, 1, 2, 7]), 'c12': (12, [10, 12])}
CASES = [(b, s) for b in BUILDS for s in SHAPES]
_ids = lambda v: 'c%de%d-%s' % (v[0] + (v[1], ))
LEVELS = 3


@pytest.fixture(autouse=True)
def _restore_switches(built_lib):
    from molgym_amd import _lib
    prev = (_lib.is_deterministic(), _lib.is_deterministic_covariant())
    yield
    _lib.set_deterministic(prev[0], covariant=prev[1])


def _pair_data(build, shape):
    canvas, counts = SHAPES[shape]
    name = f'cfg2_canvas{canvas}'
    CONFIGS.setdefault(name, dict(CONFIGS['cfg2'], canvas_size=canvas))
    ac, ref, cfg = make_pair(name, seed=300 + 10 * build[0] + canvas, num_channels_hidden=build[0], num_channels_per_element=build[1])
    data = crowded(name, counts, 71 + canvas)
    if not np.isfinite(data['adv']).all():
        data['adv'] = np.linspace(0.7, -0.4, len(data['adv']))
    return ac, ref, cfg, data


_RUNS = {}


def _run(build, shape):
    """step + backward of the product and of the float64 oracle, once per (build, shape); nothing here is changed afterwards"""
    key = (build, shape)
    if key not in _RUNS:
        from oracle.covariant_ref import parse_observations
        ac, ref, cfg, data = _pair_data(build, shape)
        B = len(data['obs'])
        g = torch.Generator().manual_seed(9)
        w = tuple(torch.randn(B, generator=g, dtype=torch.float64) * s for s in (1.0, 0.3, 0.7))
        ac.theta.grad = None
        out = ac.step(data['obs'], data['act'])
        (out['logp'].double() * w[0].cuda() + out['ent'].double() * w[1].cuda() + out['v'].double() * w[2].cuda()).sum().backward()
        torch.cuda.synchronize()
        d = parse_observations(data['obs'], cfg['zs'], cfg['canvas_size'], torch.float64)
        ccfg = ac._make_cfg(B, d['num_atoms'].numpy())
        views = {}
        for k in range(1, LEVELS):
            for l in range(5):
                for name in (f'cat_a{k}_{l}', f'w.atom{k}_{l}.mf', f'w.atom{k}_{l}.mb'):
                    views[name] = ac.workspace_view(name, ccfg).detach().cpu().clone()
        exp, want = oracle_backward(ref, data, w)
        _RUNS[key] = dict(ac=ac, ref=ref, cfg=cfg, data=data, d=d, views=views, want=want,
                          grad=ac.theta.grad.detach().cpu().clone(), theta=ac.theta.detach().cpu().clone())
    return _RUNS[key]


def _pad_to(n):
    nt = 32 if n % 32 == 0 else 24 if n % 24 == 0 else 20 if n % 20 == 0 else 8
    return (n + nt - 1) // nt * nt


def _slot(run, k, l):
    name = f'cg_model.cormorant_cg.atom_levels.{k}.cat_mix.weights.{l}'
    off, shape = run['ac'].slot_table[name]
    return name, off, shape


# ---- (a) derived weights: the numpy fold, bit for bit -----------------------------------------------------------------------------
@pytest.mark.parametrize('build', BUILDS, ids=lambda b: 'c%de%d' % b)
def test_derived_weights_are_the_folded_weights(built_lib, build):
    run = _run(build, 'c7')
    CH = build[0]
    emap = expected_map()
    for k in range(1, LEVELS):
        for l in range(5):
            _, off, (O, Q, _two) = _slot(run, k, l)
            assert Q == CH * (2 * NBLK[l] + 1)
            W = run['theta'][off:off + O * Q * 2].numpy().reshape(O, Q, 2)
            logical, serve = emap[l]
            Ws = WIDTHS[l]
            eff = np.zeros((O, CH * Ws, 2), dtype=np.float32)
            for cs, col in enumerate(logical):
                mirrored = [(c2, s) for c2, (st, s) in serve.items() if st == cs and c2 != col]
                assert len(mirrored) <= 1
                for c in range(CH):
                    v = W[:, col * CH + c, :].copy()
                    if mirrored:
                        v = v + np.float32(mirrored[0][1]) * W[:, mirrored[0][0] * CH + c, :]   # one float32 add per entry
                    eff[:, c * Ws + cs, :] = v
            N, K = 2 * O, 2 * CH * Ws
            mf = run['views'][f'w.atom{k}_{l}.mf'].numpy()
            mb = run['views'][f'w.atom{k}_{l}.mb'].numpy()
            ldf, ldb = _pad_to(N), _pad_to(K)
            assert mf.size == K * ldf and mb.size == N * ldb
            mf, mb = mf.reshape(K, ldf)[:, :N], mb.reshape(N, ldb)[:, :K]
            re, im = eff[..., 0], eff[..., 1]
            want_mf = np.zeros((K, N), dtype=np.float32)
            want_mf[0::2, 0::2], want_mf[0::2, 1::2] = re.T, im.T
            want_mf[1::2, 0::2], want_mf[1::2, 1::2] = -im.T, re.T
            want_mb = np.zeros((N, K), dtype=np.float32)
            want_mb[0::2, 0::2], want_mb[0::2, 1::2] = re, -im
            want_mb[1::2, 0::2], want_mb[1::2, 1::2] = im, re
            assert np.array_equal(mf, want_mf), (k, l)
            assert np.array_equal(mb, want_mb), (k, l)


# ---- (b) stored rows against the oracle's [ag | in | sq] picked through the map -------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_stored_rows_vs_oracle(built_lib, case):
    build, shape = case
    run = _run(build, shape)
    CH, ref, d = build[0], run['ref'], run['d']
    with torch.no_grad():
        atoms_all, edges_all, extra = ref.cg_model(d, return_all=True)
        cg = ref.cg_model.cg.to(torch.float64)
    am = d['atom_mask']
    TA = int(am.sum())
    emap = expected_map()
    worst = 0.0
    for k in range(1, LEVELS):
        with torch.no_grad():
            reps = atoms_all[k - 1]
            edge_reps = so3.scalar_times_vec(edges_all[k], extra['sph'])
            ag = so3.cg_product(cg, edge_reps, reps, 4, aggregate=True)
            sq = so3.cg_product(cg, reps, reps, 4)
        for l in range(5):
            cat = torch.cat([ag[l], reps[l], sq[l]], dim=-3)[am]   # (TA, (2 nblk + 1) CH, 2l + 1, 2), channel = part * CH + c
            logical = emap[l][0]
            Ws, nm = WIDTHS[l], 2 * l + 1
            ld = (2 * CH * Ws + 31) // 32 * 32
            got = run['views'][f'cat_a{k}_{l}'][:TA * nm * ld].view(TA, nm, ld)[:, :, :2 * CH * Ws].reshape(TA, nm, CH, Ws, 2).double()
            want = cat.reshape(TA, 2 * NBLK[l] + 1, CH, nm, 2)[:, logical].permute(0, 3, 2, 1, 4)   # (TA, m, c, cs, 2)
            err = (got - want).abs().max().item() / max(want.abs().max().item(), 1e-30) if TA else 0.0
            print(f'build {build} shape {shape} cat_a{k}_{l}: max |err| / max |want| = {err:.3e}')
            worst = max(worst, err)
            assert err < 1e-5, (k, l, err)
    assert TA == 0 or worst > 0.0


# ---- (c) gradients --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_gradients_vs_oracle_and_the_fold(built_lib, case):
    build, shape = case
    run = _run(build, shape)
    CH, want, grad = build[0], run['want'], run['grad']
    report = grad_report(grad.double(), want, run['ac'].slot_table)
    print(f'build {build} shape {shape}: worst gradient slot (err / slot max)', max(v[0] for v in report.values() if v[1] >= 1e-10))
    assert bool(torch.isfinite(grad).all())
    assert_grads(report)
    emap = expected_map()
    pairs = dropped = 0
    for k in range(1, LEVELS):
        for l in range(5):
            name, off, (O, Q, _two) = _slot(run, k, l)
            g = grad[off:off + O * Q * 2].view(O, 2 * NBLK[l] + 1, CH, 2)
            gw = want[name].grad.reshape(O, 2 * NBLK[l] + 1, CH, 2).double().cpu()
            slot_max = gw.abs().max().item()
            logical, serve = emap[l]
            for col, (st, s) in serve.items():
                if st < 0:      # a part whose block is identically zero: nothing is added; the oracle's own value is rounding
                    assert gw[:, col].abs().max().item() < 2e-4 * slot_max, (k, l, col)
                    assert (g[:, col] == 0).all(), (k, l, col)
                    dropped += 1
                elif logical[st] != col:   # mirrored onto stored column st: the same float, times s
                    assert torch.equal(g[:, col], s * g[:, logical[st]]), (k, l, col)
                    assert g[:, col].abs().max().item() > 0
                    pairs += 1
    # per level: 4 + 6 + 7 + 6 mirrored blocks and the 4 + 3 odd-l diagonals (30 of the 65 blocks are not stored)
    assert pairs == 2 * 23 and dropped == 2 * 7


# ---- (d) fold hygiene -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('build', BUILDS, ids=lambda b: 'c%de%d' % b)
def test_fold_reads_and_zeroes_every_entry_once(built_lib, build):
    ac, _, _, data = _pair_data(build, 'c7')
    batch = device_batch(ac, data)
    ac.theta.grad = torch.zeros_like(ac.theta)
    ac.invalidate_weights()
    ac.ppo_minibatch(batch, *HP, epoch_cache=True)
    torch.cuda.synchronize()
    assert ac.workspace_view('dwexp', batch.cfg).abs().max().item() > 0   # (deferred: the expanded gradients wait in the workspace)
    ac.fold_gradients()
    torch.cuda.synchronize()
    g1 = ac.theta.grad.clone()
    assert torch.isfinite(g1).all() and g1.abs().max().item() > 0
    assert ac.workspace_view('dwexp', batch.cfg).abs().max().item() == 0
    ac._ws_epoch[0]['pending'] = True   # a second fold of the same workspace adds zeros
    ac.fold_gradients()
    torch.cuda.synchronize()
    assert ac.workspace_view('dwexp', batch.cfg).abs().max().item() == 0
    assert torch.equal(ac.theta.grad, g1)


# ---- (e) ordered mode -----------------------------------------------------------------------------------------------------------
def test_ordered_mode_repeats_its_bits(built_lib):
    import molgym_amd
    ac, _, _, data = _pair_data((10, 4), 'c7')
    molgym_amd.set_deterministic(True, covariant=True)
    batch = device_batch(ac, data)
    runs = []
    for _ in range(2):
        ac.theta.grad = torch.zeros_like(ac.theta)
        stats = ac.ppo_minibatch(batch, *HP)
        torch.cuda.synchronize()
        runs.append((stats.clone(), ac.theta.grad.clone(), ac._last_out.clone()))
    assert torch.isfinite(runs[0][1]).all() and runs[0][1].abs().max().item() > 0
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)
