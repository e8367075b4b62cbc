"""The clamp and saturation branches of the action heads, against the float64 oracle.  Every other oracle comparison of the
evaluation path runs at the initialisation, where the focus and element logits are flat to 1e-2 and no clamp but the high one of a
single-entry row is reached.  Here the weights are moved until the branches are taken, and the test asserts FROM THE ORACLE that
they are before it compares anything:

  A  CovariantAC, the last Linear of phi_focus / phi_element times a gain: Categorical's clamp of q to [eps, 1 - eps], the gradient
     cut outside it, log(eps) for a clamped pick, the max subtraction -- fused heads, staged heads (network_width 256), staged heads
     under the ordered switch, staged heads with 9 symbols
  B  the GMM head: a component clamped to a standard deviation of 1e-6, alone and in a mixture; mixture logits 120 apart and
     means at tanh = +-1 exactly
  C  the orientation head with the mixer's weights times 1e-5, 1e-9 and 0: k below its clamp with a numerator that is not zero, p
     below its clamp, 0 / 0
  D  beta = +-60 and +-1000: at these weights |s|^2 stays below 0.2, so it takes 1000 to put the exponents of the Lebedev
     log-sum-exp beyond the range of expf
  E  SchNetAC: the same as A on the fused heads (canvas 7, 12), the grouped heads (canvas 20, 70), and log_stds +- 6

Rows on which float32 and float64 may sit on different sides of a clamp (`ambiguous`, tests/helpers.py::categorical_classes) get a
zero output adjoint on both sides and are left out of the output comparison; their number is capped.

Tolerances.  The additive cases (B, C, D, log_stds) and the comparison of A on the kernel's OWN logits keep the project's
(helpers.OUTPUT_TOL, assert_grads' defaults).  In the gain cases the gain multiplies the encoder's float32 rounding, so logp / ent
are conditioning-limited: the bound of each output is max(project tolerance, 4 x the deviation of a float32 copy of the ORACLE from
the float64 oracle on the same rows) -- measured from the reference alone; 4 because the kernels add in another order than torch --
under hard ceilings (logp 1e-4, ent 1e-3: a clamp branch taken wrongly misses by more than 1e-2).  The gradient keeps assert_grads'
defaults everywhere.

How the rows reach their classes (CPU calibration on the oracle, asserted again by every run).  The focus logit of an atom is first
of all a function of its species -- 0.02 between F and S at the initialisation -- and varies by 1e-4 .. 5e-3 among atoms of one
species.  One gain of a few thousand therefore clamps the mixed-species rows and leaves single-species rows inside the clamps
(species_rows), where a gain of 1e4 and more on make_batch's random species leaves no row inside them.  The element head of
make_pair is dominated by its biases (0.1 randn in both layers, times the gain): every row alike.  Both are set to zero before the
gain is applied, which leaves per-row spreads of 2e-4 .. 1e-2.  Picks are uniform draws, too rarely the improbable entry: on a few
rows they are set to the oracle's least (or most) probable valid entry (steer_picks)."""
import numpy as np
import pytest
import torch

from molgym_amd.synthetic import CONFIGS, make_batch, make_batch_internal
from oracle.covariant_ref import CategoricalRef, SO3DistRef, masked_softmax
from tests.helpers import (OUTPUT_TOL, abs1_err, add_to_slot, assert_grads, categorical_classes, crowded, float32_oracle_deviation,
                           grad_report, launch_log, make_pair, rel_err, scale_last_linear, scale_slot, sync_oracle)

pytestmark = pytest.mark.gpu
ZS16 = [0, 1, 5, 6, 7, 8, 9, 14, 15, 16, 17, 33, 34, 35, 52, 53]   # tests/test_gpu_wide_zs.py
CEILING = {'logp': 1e-4, 'ent': 1e-3, 'v': 1e-4}   # (v: no gain reaches it; its bound follows the float32 oracle like the others)
# rows of each class that a head must reach among the rows compared, and the cap on ambiguous rows, of a mini-batch of 32.  The
# three classes but `high` exclude each other, so a head claims 11 rows: the case of 16 rows is asked for half of each number,
# rounded up, and the case of 8 rows -- it cannot hold them at all -- for one row of each class.
NEED = {'pick_low': 3, 'low_other': 3, 'high': 1, 'inside': 5}
NEED_16 = {'pick_low': 2, 'low_other': 2, 'high': 1, 'inside': 3}
NEED_8 = {'pick_low': 1, 'low_other': 1, 'high': 1, 'inside': 1}
MAX_AMBIGUOUS = 4
PROJECT = {k: tol for k, (_, tol) in OUTPUT_TOL.items()}
_CACHE = {}   # oracle results shared by the launch paths of one case: computed once, never written again


class _Grad:
    def __init__(self, g):
        self.grad = g


# ---- shared machinery -------------------------------------------------------------------------------------------------------
def _loss_weights(B, keep, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(3, B, generator=g, dtype=torch.float64) * torch.tensor([[1.0], [0.3], [0.7]], dtype=torch.float64)
    w[:, ~keep] = 0.0
    return w


def _oracle_grads(ref, exp, w):
    ref.zero_grad()
    (exp['logp'] * w[0] + exp['ent'] * w[1] + exp['v'] * w[2]).sum().backward()
    return {k: _Grad(p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)) for k, p in ref.named_parameters()}


def _class_counts(c, ambiguous):
    ok = ~ambiguous
    return {'pick_low': int((c['pick_low'] & ok).sum()), 'low_other': int((c['low'] & ~c['pick_low'] & ok).sum()),
            'high': int((c['high'] & ok).sum()), 'inside': int((c['inside'] & (c['spread'] >= 1.0) & ok).sum())}


def _assert_reached(tag, heads, need=NEED):
    """`heads`: {name: categorical_classes(...)} of the focus and the element head of one mini-batch.  -> the rows to compare"""
    ambiguous = torch.zeros_like(next(iter(heads.values()))['ambiguous'])
    for c in heads.values():
        ambiguous |= c['ambiguous']
    counts = {name: _class_counts(c, ambiguous) for name, c in heads.items()}
    print(f'{tag}: ambiguous rows {int(ambiguous.sum())} of {len(ambiguous)}, classes {counts}')
    assert int(ambiguous.sum()) <= MAX_AMBIGUOUS * len(ambiguous) // 32, (tag, ambiguous.nonzero().flatten().tolist())
    for name, cnt in counts.items():
        for k, n in need.items():
            assert cnt[k] >= n, (tag, name, k, cnt)
    return ~ambiguous, counts


def _gain_bounds(tag, ref, data, keep, exp):
    dev = float32_oracle_deviation(ref, data, keep, exp64=exp)
    bounds = {k: max(PROJECT[k], 4.0 * dev[k]) for k in PROJECT}
    print(f'{tag}: float32 oracle deviation {dev}, bounds {bounds}')
    for k, b in bounds.items():
        assert b <= CEILING[k], (tag, k, dev, 'lower the gain; the ceiling stays')
    return bounds


def _hip_step(ac, data):
    """the forward under the launch log; the callers read the head workspace before the backward reuses anything"""
    ac.theta.grad = None
    with launch_log() as log:
        out = ac.step(data['obs'], data['act'])
    return out, log


def _hip_backward(ac, out, w):
    wd = w.cuda()
    (out['logp'].double() * wd[0] + out['ent'].double() * wd[1] + out['v'].double() * wd[2]).sum().backward()
    torch.cuda.synchronize()
    return ac.theta.grad.detach().double().cpu()


def _compare(tag, ac, out, grad, exp, grads, keep, bounds=PROJECT):
    for k in PROJECT:
        assert torch.isfinite(out[k]).all(), (tag, k)
    assert torch.isfinite(grad).all(), tag
    errs = {k: rel_err(out[k].detach().cpu()[keep], exp[k].detach()[keep], **OUTPUT_TOL[k][0]) for k in PROJECT}
    report = grad_report(grad, grads, ac.slot_table)
    print(f'{tag}: errors {errs} within {bounds}; worst gradient slot (err / slot max)',
          max((v[0], k) for k, v in report.items() if v[1] >= 1e-10))
    for k, e in errs.items():
        assert e < bounds[k], (tag, k, e, bounds[k])
    assert_grads(report)
    return report


class _ordered:
    """the ordered switch of CovariantAC for the block (mg_cov_set_ordered returns the previous value)"""

    def __init__(self, ac, on):
        self.lib, self.on = ac._L(), on

    def __enter__(self):
        self.prev = self.lib.mg_cov_set_ordered(1) if self.on else None

    def __exit__(self, *exc):
        if self.on:
            self.lib.mg_cov_set_ordered(self.prev)
        return False


PATHS = {'fused': (128, False), 'staged': (256, False), 'staged_ordered': (256, True)}


def _assert_path(log, path):
    if path == 'fused':
        assert log.ran('k_heads_fwd') and not log.ran('k_focus_head') and not log.ran('k_element_head')
    else:
        assert log.ran('k_focus_head') and log.ran('k_element_head') and log.ran('k_gmm') and log.ran('k_so3')
        assert not log.ran('k_heads_fwd')


def _head_views(ac, exp, B):
    """(parts (6, B), logz (B,)) of the forward just run, copied"""
    ccfg = ac._make_cfg(B, exp['data']['num_atoms'].numpy())
    return ac.workspace_view('parts', ccfg)[:6 * B].view(6, B).double().cpu().clone(), ac.workspace_view('logz', ccfg)[:B].double().cpu().clone()


# ---- A. peaked categoricals ---------------------------------------------------------------------------------------------------
# (make_pair seed, make_batch seed, focus gain, element gain) per (network_width, symbols): found on the CPU, on the oracle
PEAKED = {(128, 3): (12, 3, 5.0e3, 3.0e3), (256, 3): (12, 3, 5.0e3, 7.0e3), (256, 9): (24, 3, 5.0e3, 7.0e3)}


def species_rows(data, Z, every):
    """make_batch draws every atom's species at random.  Here every `every`-th row holds atoms of ONE species (their focus logits
    differ by their surroundings alone: inside the clamps at the gains used) and every other row of two atoms or more holds at
    least two species (a gap that the gain turns into a clamped entry).  Positions, bags and actions stay."""
    obs = []
    for b, (canvas, bag) in enumerate(data['obs']):
        labels = [label for label, _ in canvas]
        n = sum(1 for label in labels if label != 0)
        if b % every == 0:
            labels[:n] = [1 + (b // every) % (Z - 1)] * n
        elif n >= 2 and len(set(labels[:n])) == 1:
            labels[1] = labels[0] % (Z - 1) + 1
        obs.append((tuple((label, xyz) for label, (_, xyz) in zip(labels, canvas)), bag))
    return dict(data, obs=obs)


def peaked_covariant(width, Z, B, monkeypatch=None, device='cuda:0'):
    """-> (agent, oracle, data) of case A.  Runs on the CPU too (the agent then only holds the weights)."""
    seed, dseed, gf, ge = PEAKED[(width, Z)]
    name = 'cfg2'
    if Z != 3:
        name = f'edges_z{Z}'
        (monkeypatch.setitem if monkeypatch is not None else (lambda d, k, v: d.__setitem__(k, v)))(
            CONFIGS, name, dict(zs=ZS16[:Z], canvas_size=7, batch=16, bag_scale=5, beta=-10.0))
    ac, ref, cfg = make_pair(name, seed=seed, device=device, network_width=width)
    for layer in (0, 1):   # (exactly zero; the docstring)
        off, shape = ac.slot_table[f'phi_element.layers.{layer}.bias']
        add_to_slot(ac, f'phi_element.layers.{layer}.bias', -ac.theta.detach()[off:off + shape[0]].double().cpu())
    scale_last_linear(ac, ref, ('phi_focus', 'phi_element'), (gf, ge))
    every = 3 if B >= 32 else 2
    # atom counts: an empty, a one-atom and a full canvas first, then 2 .. 7 in turn, three atoms or more on the single-species rows
    counts = [0, 1, 7] + [2 + (b * 5) % 6 for b in range(3, B)]
    counts = [max(n, 3) if b % every == 0 and b else n for b, n in enumerate(counts)]
    data = species_rows(crowded(name, counts, dseed), Z, every)
    if Z > 3:
        # eight species give a mixed row several gaps, one of which is near the clamp on too many rows: the mixed rows hold the
        # lightest and the heaviest species only.  (A gain above 1e4 costs too much of logp's float32 accuracy: the ceiling.)
        # Among eight symbols one is clamped wherever any is: every other bag keeps two symbols, the picked one and the next.
        obs = []
        for b, (canvas, bag) in enumerate(data['obs']):
            if b % every:
                labels = [0 if label == 0 else (1 if label <= Z // 2 else Z - 1) for label, _ in canvas]
                if counts[b] >= 2 and labels[0] == labels[1]:
                    labels[1] = Z - labels[0]
                canvas = tuple((label, xyz) for label, (_, xyz) in zip(labels, canvas))
            if b % 2:
                e = int(round(data['act'][b, 1]))
                bag = tuple(max(c, 1) if i in (e, e % (Z - 1) + 1) else 0 for i, c in enumerate(bag))
            obs.append((canvas, bag))
        data = dict(data, obs=obs)
    rows = np.arange(B)
    if Z > 3:   # sixteen rows, eleven of them claimed by each head: the picks of the rows that are to be clamped alternate
        return ac, ref, steer_picks(ref, data, rows[rows % 4 == 1], rows[rows % 4 == 2], rows[rows % 4 == 3], rows[rows % 4 == 0])
    mixed = [b for b in range(B) if b % every and counts[b] >= 2]
    return ac, ref, steer_picks(ref, data, mixed[0::3], rows[rows % 4 >= 2])


def steer_picks(ref, data, focus_rows, element_rows, focus_most=(), element_most=()):
    """make_batch picks uniformly, which too rarely is the improbable entry: on `focus_rows` act[:, 0] becomes the oracle's LEAST
    probable valid atom, then -- the element logits follow the focused atom -- on `element_rows` act[:, 1] its least probable valid
    element; on the `_most` rows the most probable one.  (The order of a row's logits does not depend on the gain.)"""
    act = np.array(data['act'], dtype=np.float64)
    for col, key, mask_key, rows, most in ((0, 'focus_logits', 'focus_mask', focus_rows, focus_most),
                                           (1, 'element_logits', 'element_mask', element_rows, element_most)):
        with torch.no_grad():
            exp = ref.step(data['obs'], act, dtype=torch.float64, return_internals=True)
        mask = exp['data'][mask_key]
        worst = torch.where(mask, exp[key], torch.full_like(exp[key], float('inf'))).argmin(-1).numpy()
        best = torch.where(mask, exp[key], torch.full_like(exp[key], -float('inf'))).argmax(-1).numpy()
        act[rows, col] = worst[rows]
        if len(most):
            act[most, col] = best[most]
    return dict(data, act=act)


def peaked_oracle(ref, data, internal=False):
    """the float64 oracle on a gain case -> (outputs, {focus / element: categorical_classes})"""
    act = torch.as_tensor(np.asarray(data['act']))
    if internal:
        exp, heads = _internal_oracle(ref, data)
    else:
        exp = ref.step(data['obs'], data['act'], dtype=torch.float64, return_internals=True)
        d = exp['data']
        heads = {'focus': categorical_classes(exp['focus_logits'], d['focus_mask'], act[:, 0].round()),
                 'element': categorical_classes(exp['element_logits'], d['element_mask'], act[:, 1].round())}
    return exp, heads


def _peaked_case(tag, key, ref, data, seed, need=NEED, internal=False):
    if key not in _CACHE:
        exp, heads = peaked_oracle(ref, data, internal)
        keep, counts = _assert_reached(tag, heads, need)
        w = _loss_weights(len(keep), keep, seed)
        grads = _oracle_grads(ref, exp, w)
        bounds = _gain_bounds(tag, ref, data, keep, exp)
        _CACHE[key] = (exp, keep, w, grads, bounds)
    return _CACHE[key]


def _own_logits_check(tag, ac, out, parts, data, Z):
    """parts[0, 1, 4, 5] -- the two Categoricals' log-probabilities and entropies -- against a float64 CategoricalRef on the
    KERNEL's logits (the packed copy behind out['dists'], laid out as tests/test_gpu_draws.py::_cov_replay reads it): no encoder
    rounding in this comparison, so the project's tolerances hold at any gain"""
    B, N = len(data['obs']), len(data['obs'][0][0])
    blk = out['dists']._block.detach().double().cpu()
    logit_f = blk[:B * N].view(B, N)
    natoms = blk[B * N:B * N + B].round().long()
    logit_e = blk[B * N + B:B * N + B + B * Z].view(B, Z)
    act = torch.as_tensor(np.asarray(data['act']))
    fmask = torch.arange(N)[None, :] < natoms.clamp(min=1)[:, None]
    emask = torch.tensor([o[1] for o in data['obs']]) > 0
    worst = {}
    ambiguous = torch.zeros(B, dtype=torch.bool)
    sides = []
    for i, (logits, mask, col) in enumerate(((logit_f, fmask, 0), (logit_e, emask, 1))):
        logits = torch.where(mask, logits, torch.zeros_like(logits))     # (an empty canvas' lone entry: whatever it holds cancels)
        picks = act[:, col].round().long()
        ambiguous |= categorical_classes(logits, mask, picks)['ambiguous']
        dist = CategoricalRef(masked_softmax(logits, mask))
        sides.append((dist.log_prob(picks), dist.entropy()))
    keep = ~ambiguous
    assert int(ambiguous.sum()) <= MAX_AMBIGUOUS * B // 32, (tag, ambiguous.nonzero().flatten().tolist())
    for i, (lp, ent) in enumerate(sides):
        worst[f'lp{i}'] = abs1_err(parts[i][keep], lp[keep])
        worst[f'ent{i}'] = rel_err(parts[4 + i][keep], ent[keep], **OUTPUT_TOL['ent'][0])
    print(f'{tag}: own-logits comparison on {int(keep.sum())} rows {worst}')
    for i in range(2):
        assert worst[f'lp{i}'] < 1e-5 and worst[f'ent{i}'] < OUTPUT_TOL['ent'][1], (tag, worst)


@pytest.mark.parametrize('path', list(PATHS))
def test_peaked_categoricals(built_lib, path):
    width, ordered = PATHS[path]
    tag = f'peaked[{path}]'
    ac, ref, data = peaked_covariant(width, 3, 32)
    exp, keep, w, grads, bounds = _peaked_case(tag, ('A', width, 3), ref, data, seed=11)
    with _ordered(ac, ordered):
        out, log = _hip_step(ac, data)
        parts, _ = _head_views(ac, exp, 32)
        grad = _hip_backward(ac, out, w)
    _assert_path(log, path)
    _own_logits_check(tag, ac, out, parts, data, 3)
    _compare(tag, ac, out, grad, exp, grads, keep, bounds)


def test_peaked_categoricals_nine_symbols(built_lib, monkeypatch):
    """k_element_head<true> and its adjoint (Z > 8: the mask as a bit set, the logits read where they lie), staged heads, B = 16"""
    tag = 'peaked[staged, Z=9]'
    ac, ref, data = peaked_covariant(256, 9, 16, monkeypatch)
    exp, keep, w, grads, bounds = _peaked_case(tag, ('A', 256, 9), ref, data, seed=12, need=NEED_16)
    out, log = _hip_step(ac, data)
    parts, _ = _head_views(ac, exp, 16)
    grad = _hip_backward(ac, out, w)
    _assert_path(log, 'staged')
    _own_logits_check(tag, ac, out, parts, data, 9)
    _compare(tag, ac, out, grad, exp, grads, keep, bounds)


# ---- B. the GMM head ----------------------------------------------------------------------------------------------------------
def gmm_case(kind, width, device='cuda:0'):
    G = 1 if kind == 'clamped_alone' else 3
    ac, ref, cfg = make_pair('cfg2', seed=21, device=device, network_width=width, num_gaussians=G)
    if kind in ('clamped_component', 'clamped_alone'):
        off, _ = ac.slot_table['distance_log_stds']
        add_to_slot(ac, 'distance_log_stds', [-20.0 - ac.theta[off].item()] + [0.0] * (G - 1))
    else:  # mixture logits (0, +60, -60), mean pre-activations (+12, -12, 0): tanhf(+-12) is +-1 exactly in float32
        add_to_slot(ac, 'phi_d.layers.1.bias', [0.0, 60.0, -60.0, 12.0, -12.0, 0.0])
    sync_oracle(ac, ref)
    data = make_batch(24, cfg['canvas_size'], cfg['zs'], seed=22)
    if kind != 'saturated':
        # alone: logp = -d^2 / 2e-12 with d = x - mean, a difference of float32 numbers near 1.5 (2^-23 each): the relative error of
        # logp is twice that of d, so 1e-5 needs |d| well above 0.05.  In the mixture: the clamped component's responsibility is
        # exp(-d^2 / 2e-12) of the others', zero unless |d| < 1e-4.  The mean does not depend on x: distances close to it move out.
        margin = 0.15 if kind == 'clamped_alone' else 0.01
        mean = _gmm_means(ref, data)[:, 0]
        x = torch.as_tensor(data['act'][:, 2])
        data['act'][:, 2] = torch.where((x - mean).abs() < margin, mean + torch.where(x < mean, -margin, margin), x).numpy()
    return ac, ref, data


def _gmm_means(ref, data):
    seen = []
    hook = ref.phi_d.register_forward_hook(lambda m, i, o: seen.append(o.detach()))
    with torch.no_grad():
        ref.step(data['obs'], data['act'], dtype=torch.float64)
    hook.remove()
    G = ref.num_gaussians
    return torch.tanh(seen[0][:, G:]) * (ref.max_distance - ref.min_distance) / 2 + (ref.max_distance + ref.min_distance) / 2


def _gmm_oracle(key, kind, ref, data):
    if key not in _CACHE:
        B = len(data['obs'])
        mean = _gmm_means(ref, data)
        exp = ref.step(data['obs'], data['act'], dtype=torch.float64, return_internals=True)
        x = exp['a'][:, 2]
        if kind == 'clamped_component':
            assert (x - mean[:, 0]).abs().min().item() > 1e-3    # (gmm_case)
        elif kind == 'clamped_alone':
            assert (x - mean[:, 0]).abs().min().item() > 0.1     # (gmm_case)
            assert exp['logp'].max().item() < -1e9
        else:
            assert (x > ref.max_distance).any() and (x < ref.max_distance).any()      # actions beyond every mean's range
            assert (mean[:, 0] - ref.max_distance).abs().max().item() < 1e-8 and (mean[:, 1] - ref.min_distance).abs().max().item() < 1e-8
        keep = torch.ones(B, dtype=torch.bool)
        w = _loss_weights(B, keep, 23)
        _CACHE[key] = (exp, keep, w, _oracle_grads(ref, exp, w))
    return _CACHE[key]


@pytest.mark.parametrize('path', list(PATHS))
@pytest.mark.parametrize('kind', ['clamped_component', 'clamped_alone', 'saturated'])
def test_gmm_head(built_lib, kind, path):
    """fmaxf(expf(logstd), 1e-6f) with the gate on the log-std gradient (k_gmm / k_gmm_bwd / k_gmm_logstd_bwd_ord and the
    copies inside k_heads_fwd / k_heads_bwd), tanhf at +-1, both max-subtracted log-sum-exps.  Additive changes: project tolerances."""
    width, ordered = PATHS[path]
    tag = f'gmm[{kind}, {path}]'
    ac, ref, data = gmm_case(kind, width)
    exp, keep, w, grads = _gmm_oracle(('B', kind, width), kind, ref, data)
    with _ordered(ac, ordered):
        out, log = _hip_step(ac, data)
        grad = _hip_backward(ac, out, w)
    _assert_path(log, path)
    _compare(tag, ac, out, grad, exp, grads, keep)
    if kind != 'saturated':   # the clamped component's log-std gradient: exactly zero on both sides
        off, _ = ac.slot_table['distance_log_stds']
        assert grad[off].item() == 0.0 and grads['distance_log_stds'].grad[0].item() == 0.0
        if kind == 'clamped_component':
            assert grad[off + 1:off + 3].abs().min().item() > 0.0


# ---- C. the orientation head with a vanishing mixer ---------------------------------------------------------------------------
def so3_case(s, beta, width, device='cuda:0'):
    ac, ref, cfg = make_pair('cfg2', seed=31, beta=beta, device=device, network_width=width)
    for l in range(5):
        scale_slot(ac, f'cg_mix.cat_mix.weights.{l}', s)
    sync_oracle(ac, ref)
    return ac, ref, make_batch(24, cfg['canvas_size'], cfg['zs'], seed=32)


def _so3_oracle(key, s, ref, data):
    if key not in _CACHE:
        B = len(data['obs'])
        exp = ref.step(data['obs'], data['act'], dtype=torch.float64, return_internals=True)
        empty = exp['data']['empty']
        k = sum(p.sum(dim=-3).square().sum(dim=(-1, -2)) for p in exp['cond_cov']).detach()
        keep = torch.ones(B, dtype=torch.bool)
        assert (~empty).sum() >= 16 and empty.any()
        assert k[~empty].max().item() < 1e-10 / 16, k               # k under its clamp on every non-empty row, clear of it
        if s != 0:
            assert k[~empty].min().item() > 0
        else:
            assert k.abs().max().item() == 0
        if ref.beta is None:   # p = |sum a Y|^2 / max(k, 1e-10) against ITS clamp at 1e-10
            with torch.no_grad():
                p = SO3DistRef(exp['cond_cov'], ref.cg, ref.max_sh, None, empty)._s2(exp['a'][:, 3:6]).detach()
            near = (p >= 1e-10 / 16) & (p <= 16e-10) & ~empty
            keep = ~near
            print(f'so3[s={s:g}]: p of the non-empty rows {p[~empty].min().item():.3g} .. {p[~empty].max().item():.3g}, '
                  f'{int(near.sum())} rows near the clamp left out')
            if s == 1e-5:
                assert (p[~empty & keep] > 16e-10).sum() >= 12   # clamped k, P not zero, p above its clamp
            else:
                assert (p[~empty & keep] < 1e-10 / 16).all() and (~empty & keep).sum() >= 8
        w = _loss_weights(B, keep, 33)
        _CACHE[key] = (exp, keep, w, _oracle_grads(ref, exp, w))
    return _CACHE[key]


@pytest.mark.parametrize('path', ['fused', 'staged'])
@pytest.mark.parametrize('beta', ['cfg', None])
@pytest.mark.parametrize('s', [1e-5, 1e-9, 0.0])
def test_orientation_head_with_vanishing_mixer(built_lib, s, beta, path):
    """invk = 1 / fmaxf(k, 1e-10f) with kpass, logf(fmaxf(p, 1e-10f)) with wa = 0 below the clamp, the Lebedev log-sum-exp of
    a flat density, and 0 * inf / 0 / 0 at s = 0 (k_so3 / k_so3_bwd and their copies in the fused heads)"""
    width, _ = PATHS[path]
    tag = f'so3[s={s:g}, beta={beta}, {path}]'
    ac, ref, data = so3_case(s, beta, width)
    exp, keep, w, grads = _so3_oracle(('C', s, beta, width), s, ref, data)
    out, log = _hip_step(ac, data)
    parts, logz = _head_views(ac, exp, 24)
    grad = _hip_backward(ac, out, w)
    _assert_path(log, path)
    assert torch.isfinite(parts).all() and torch.isfinite(logz).all()
    assert abs1_err(parts[3][keep], exp['logps'][3].detach()[keep]) < 1e-5
    if beta is not None:
        assert rel_err(logz, exp['log_z'].detach()) < 1e-5
    _compare(tag, ac, out, grad, exp, grads, keep)
    if s == 0.0 or (s == 1e-9 and beta is None):   # nothing reaches the mixer through a clamp: exactly zero on both sides
        for l in range(5):
            name = f'cg_mix.cat_mix.weights.{l}'
            off, shape = ac.slot_table[name]
            assert grads[name].grad.abs().max().item() == 0.0
            assert grad[off:off + int(np.prod(shape))].abs().max().item() == 0.0, name


# ---- D. large |beta| ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path', ['fused', 'staged'])
@pytest.mark.parametrize('beta', [-60.0, 60.0, -1000.0, 1000.0])
def test_large_beta(built_lib, beta, path):
    """the running max of the Lebedev log-sum-exp.  |s|^2 may reach 25 / (4 pi), but at the initialisation it stays below 0.2:
    beta = +-60 gives exponents of 12, +-1000 exponents up to 160 -- beyond expf without the running max"""
    width, _ = PATHS[path]
    tag = f'beta[{beta:g}, {path}]'
    ac, ref, cfg = make_pair('cfg2', seed=41, beta=beta, network_width=width)
    data = make_batch(24, cfg['canvas_size'], cfg['zs'], seed=42)
    key = ('D', beta, width)
    if key not in _CACHE:
        exp = ref.step(data['obs'], data['act'], dtype=torch.float64, return_internals=True)
        keep = torch.ones(24, dtype=torch.bool)
        w = _loss_weights(24, keep, 43)
        _CACHE[key] = (exp, keep, w, _oracle_grads(ref, exp, w))
    exp, keep, w, grads = _CACHE[key]
    unnorm = (exp['logps'][3] + exp['log_z']).detach()       # -beta |s|^2 at the action
    print(f'{tag}: log_z {exp["log_z"].min().item():.1f} .. {exp["log_z"].max().item():.1f}, exponent at the action '
          f'{unnorm.min().item():.1f} .. {unnorm.max().item():.1f}')
    if abs(beta) > 100:   # the exponents pass the range of float32 expf (overflow above 88.7, zero below -87.3 without denormals)
        assert max(exp['log_z'].abs().max().item(), unnorm.abs().max().item()) > 88.7
    out, log = _hip_step(ac, data)
    parts, logz = _head_views(ac, exp, 24)
    grad = _hip_backward(ac, out, w)
    _assert_path(log, path)
    assert torch.isfinite(logz).all()
    assert rel_err(logz, exp['log_z'].detach()) < 1e-5
    assert abs1_err(parts[3] + logz, unnorm) < 1e-5     # (the exponent itself: its difference with log_z cancels up to 160 - 150)
    _compare(tag, ac, out, grad, exp, grads, keep)


# ---- E. SchNetAC ------------------------------------------------------------------------------------------------------------------
# (canvas, B): (_pair seed, data seed, gain of phi_focus / phi_element / phi_kappa, forward kernel, minimum class counts)
INTERNAL = {
    (7, 32): (3, 5, (50.0, 50.0, 200.0), 'k_int_heads_fwd_pre<8>', NEED),
    (12, 32): (3, 5, (50.0, 100.0, 200.0), 'k_int_heads_fwd_pre<16>', NEED),
    (20, 32): (3, 5, (50.0, 50.0, 200.0), 'k_int_heads_eval<1>', NEED),
    (70, 8): (3, 5, (200.0, 100.0, 200.0), 'k_int_heads_eval<2>', NEED_8),
}


def internal_case(canvas, B, device='cuda:0', gains=None):
    """-> (agent, oracle, data) of case E.  Atom counts: an empty and a full canvas, the molecules of one to three atoms whose
    focus logits stay inside the clamps at these gains, and sizes up to the canvas (above 64 atoms at canvas 70).  Of every four
    rows, one picks the oracle's least probable atom and element and one its most probable: a uniform pick among 20 or 70 atoms
    is the clamped one on nearly every row."""
    from molgym_amd.synthetic import make_canvas
    from tests.test_gpu_internal import ZS, _pair
    seed, dseed, g, _, _ = INTERNAL[(canvas, B)]
    ac, ref = _pair(seed, 128, canvas) if device != 'cpu' else _pair_cpu(seed, 128, canvas)
    scale_last_linear(ac, None, ('phi_focus', 'phi_element', 'phi_kappa'), gains or g)
    ref.load_state_dict({k: v.double().cpu() for k, v in ac.export_state_dict().items()}, strict=True)
    small = [0, canvas, 3, 2, canvas - 2, 3, canvas - 4, 2]
    counts = small + [(3, 2, 4, max(canvas // 2, 3), canvas - 1, 3, 5, canvas)[b % 8] for b in range(8, B)]
    data = make_batch_internal(B, canvas, ZS, seed=dseed)
    rng = np.random.default_rng(dseed + 1)
    obs = []
    for b, n in enumerate(counts):
        obs.append((make_canvas(rng, n, canvas, len(ZS)), data['obs'][b][1]))
        data['act'][b, 1] = rng.integers(0, max(n, 1))
    data = species_rows(dict(data, obs=obs), len(ZS), 3 if B >= 32 else 2)
    act = np.array(data['act'], dtype=np.float64)
    rows = np.arange(B)
    for col, key in ((1, 'focus'), (2, 'element')):     # (the element logits follow the focused atom: one head after the other)
        logits, mask = _internal_logits(ref, dict(data, act=act))[key]
        least = torch.where(mask, logits, torch.full_like(logits, float('inf'))).argmin(-1).numpy()
        most = torch.where(mask, logits, torch.full_like(logits, -float('inf'))).argmax(-1).numpy()
        act[rows % 4 == 1, col] = least[rows % 4 == 1]
        act[rows % 4 == 3, col] = most[rows % 4 == 3]
    return ac, ref, dict(data, act=act)


def _pair_cpu(seed, width, canvas):
    """tests/test_gpu_internal.py::_pair with the agent's weights on the host (calibration of the cases without a device)"""
    from molgym_amd.agents.internal import SchNetAC
    from molgym_amd.spaces import ActionSpace, ObservationSpace
    from oracle.internal_ref import SchNetACRef
    from tests.test_gpu_internal import ZS
    torch.manual_seed(seed)
    ac = SchNetAC(ObservationSpace(canvas, ZS), ActionSpace(ZS), (0.8, 1.8), width, device='cpu')
    with torch.no_grad():
        g = torch.Generator().manual_seed(seed + 1)
        for name, (off, shape) in ac.slot_table.items():
            n = int(np.prod(shape))
            if name.endswith('bias'):
                ac.theta[off:off + n] = (0.1 * torch.randn(n, generator=g)).to(ac.theta)
    return ac, SchNetACRef(ZS, canvas, (0.8, 1.8), width).double()


def _internal_logits(ref, data, grad=False):
    """SchNetACRef.step with the logits of its heads caught on the way -> {focus / element: (logits, mask), kappa: gap, exp, natoms}"""
    seen = {'focus': [], 'element': [], 'kappa': []}
    hooks = [getattr(ref, 'phi_' + k).register_forward_hook(lambda m, i, o, k=k: seen[k].append(o.detach())) for k in seen]
    with torch.set_grad_enabled(grad):
        exp = ref.step(data['obs'], data['act'], dtype=torch.float64)
    for h in hooks:
        h.remove()
    N = ref.num_atoms
    natoms = torch.tensor([sum(1 for label, _ in canvas if label != 0) for canvas, _ in data['obs']])
    fmask = torch.arange(N)[None, :] < natoms.clamp(min=1)[:, None]
    emask = torch.tensor([o[1] for o in data['obs']]) > 0
    return {'focus': (seen['focus'][0].squeeze(-1), fmask), 'element': (seen['element'][0], emask), 'exp': exp, 'natoms': natoms,
            'kappa': (seen['kappa'][0] - seen['kappa'][1]).squeeze(-1).abs()[natoms >= 3]}


def _internal_oracle(ref, data):
    """-> (outputs, classes of the two Categoricals)"""
    r = _internal_logits(ref, data, grad=True)
    act = torch.as_tensor(np.asarray(data['act']))
    heads = {'focus': categorical_classes(*r['focus'], act[:, 1].round()), 'element': categorical_classes(*r['element'], act[:, 2].round())}
    # an empty canvas' focus term is masked out of logp and ent (action_mask): its row claims no focus class
    for k in ('low', 'pick_low', 'high', 'ambiguous'):
        heads['focus'][k] = heads['focus'][k] & (r['natoms'] > 0)
    exp = r['exp']
    exp['kappa_gap'] = r['kappa']
    return exp, heads


def _internal_run(tag, ac, ref, data, exp, keep, w, grads, bounds, kernel):
    ac.theta.grad = None
    with launch_log() as log:
        out = ac.step(data['obs'], data['act'])
    grad = _hip_backward(ac, out, w)
    assert log.ran(kernel), (kernel, sorted(set(log.names)))
    _compare(tag, ac, out, grad, exp, grads, keep, bounds)


@pytest.mark.parametrize('canvas,B', list(INTERNAL))
def test_internal_peaked_heads(built_lib, canvas, B):
    """categorical_fwd / bwd of SchNetAC's heads: the fused k_int_heads_fwd_pre<8> / <16> (canvas 7 / 12), the grouped k_int_heads_eval<1>
    (canvas 20) and <2> with categorical_*_wave<2> (canvas 70, molecules above 64 atoms).  The kappa head is a two-way log-softmax
    without a clamp: its logits a large gap apart, everything finite."""
    tag = f'internal[canvas {canvas}]'
    kernel, need = INTERNAL[(canvas, B)][3:]
    ac, ref, data = internal_case(canvas, B)
    exp, keep, w, grads, bounds = _peaked_case(tag, ('E', canvas, B), ref, data, seed=51, need=need, internal=True)
    print(f'{tag}: kappa logit gaps up to {exp["kappa_gap"].max().item():.1f}')
    assert exp['kappa_gap'].max().item() > 16.0     # (beyond -log(eps): the smaller term of the two-way log-sum-exp rounds away in float32)
    if canvas == 70:
        assert max(sum(1 for label, _ in c if label != 0) for c, _ in data['obs']) > 64
    _internal_run(tag, ac, ref, data, exp, keep, w, grads, bounds, kernel)


@pytest.mark.parametrize('shift', [6.0, -6.0])
def test_internal_wide_and_narrow_gaussians(built_lib, shift):
    """log_stds +- 6 (no clamp: exp(1e-6 + log_std) in the reference): standard deviations of 60 .. 100 and of 4e-4 .. 6e-4.
    On the agent and mini-batch that tests/test_gpu_internal.py holds to 1e-5: with _pair(7) and make_batch_internal(24, 7, ZS, 8)
    logp and ent passed and v -- which no log_std reaches -- missed 1e-5 at 1.28e-5, as the float32 oracle's own v does on
    such mini-batches (1.1e-5 in test_internal_peaked_heads at canvas 7; the comment at tests/test_gpu_internal.py:75)."""
    from tests.test_gpu_internal import ZS, _pair
    tag = f'internal[log_stds {shift:+g}]'
    ac, ref = _pair(0, 128, 7)       # (agent and mini-batch of tests/test_gpu_internal.py::test_outputs_and_gradients_match_oracle)
    add_to_slot(ac, 'log_stds', shift)
    ref.load_state_dict({k: v.double().cpu() for k, v in ac.export_state_dict().items()}, strict=True)
    data = make_batch_internal(24, 7, ZS, seed=4)
    exp = ref.step(data['obs'], data['act'], dtype=torch.float64)
    keep = torch.ones(24, dtype=torch.bool)
    w = _loss_weights(24, keep, 52)
    grads = _oracle_grads(ref, exp, w)
    _internal_run(tag, ac, ref, data, exp, keep, w, grads, PROJECT, 'k_int_heads_fwd_pre<8>')
