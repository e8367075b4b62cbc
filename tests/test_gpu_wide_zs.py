"""Element sets of 9 .. 16 symbols (MG_MAX_Z = 16) in both agents, against the float64 oracles: action evaluation and its
gradients, the PPO step in graph and stream form, sampling, device canvases, and the refusals past the limit.

Every batch holds what a kernel that still thinks in eight symbols gets wrong and the oracle does not: canvas atoms whose label
index is >= 8, a sample whose bag is zero at the indices 1..7 and positive only from 8 on, chosen elements at index 8 and at index
Z - 1 (each with a positive bag count), and an empty canvas."""
import ctypes as C

import numpy as np
import pytest
import torch

from molgym_amd import _lib
from molgym_amd.spaces import ActionSpace, ObservationSpace
from molgym_amd.synthetic import CONFIGS
from oracle.internal_ref import SchNetACRef
from tests.helpers import assert_grads, grad_report, make_pair, oracle_backward, rel_err

pytestmark = pytest.mark.gpu
ZS16 = [0, 1, 5, 6, 7, 8, 9, 14, 15, 16, 17, 33, 34, 35, 52, 53]   # all below SchNet's embedding table of 100 rows


def _cov_pair(monkeypatch, Z, N, seed, **kw):
    """make_pair on the first Z symbols of ZS16 (cfg5's bag scale and beta unless overridden)"""
    name = f'zs{Z}_{N}'
    monkeypatch.setitem(CONFIGS, name, dict(zs=ZS16[:Z], canvas_size=N, batch=16, bag_scale=20, beta=-10.0))
    return make_pair(name, seed=seed, **kw)


def _canvas(rng, n, N, Z, first):
    """synthetic.make_canvas's random walk (bonds U(1.10, 2.10), no pair closer than 0.6); the first atom's label is `first`
    (an index >= 8), the others are drawn from all real symbols"""
    pos = np.zeros((max(n, 1), 3))
    k = 0
    while k < n:
        if k:
            v = rng.normal(size=3)
            cand = pos[rng.integers(k)] + rng.uniform(1.10, 2.10) * v / np.linalg.norm(v)
            if np.min(np.linalg.norm(pos[:k] - cand, axis=1)) < 0.6:
                continue
            pos[k] = cand
        k += 1
    labels = rng.integers(1, Z, size=n)
    if n:
        labels[0] = first
    return tuple([(int(l), tuple(float(x) for x in p)) for l, p in zip(labels, pos[:n])] + [(0, (0.0, 0.0, 0.0))] * (N - n))


def _batch(Z, N, counts, seed, internal=False):
    """observations with the given atom counts, valid actions (covariant: 6 columns; SchNetAC: 7) and PPO loss inputs.
    Sample 0: a bag that is positive only at the indices >= 8, element 8 chosen.  Sample 1: element Z - 1 chosen.  The others: a
    random bag, an element it holds.  Every non-empty canvas starts with an atom of label >= 8."""
    assert Z > 8 and len(counts) >= 2 and 0 in counts
    rng = np.random.default_rng(seed)
    B = len(counts)
    obs = []
    act = np.zeros((B, 7 if internal else 6))
    for b, n in enumerate(counts):
        if b == 0:
            bag = np.zeros(Z, dtype=np.int64)
            bag[8:] = rng.integers(1, 4, size=Z - 8)
            element = 8
        else:
            bag = rng.integers(0, 4, size=Z)
            bag[0] = 0
            element = Z - 1 if b == 1 else int(rng.integers(1, Z))
            bag[element] = max(bag[element], 1)
        obs.append((_canvas(rng, int(n), N, Z, 8 + (b % (Z - 8))), tuple(int(x) for x in bag)))
        focus = max(int(n) - 1, 0) if b % 2 else rng.integers(0, max(int(n), 1))
        if internal:
            act[b, 1:] = (focus, element, rng.uniform(1.1, 2.1), rng.uniform(0.3, np.pi - 0.3), rng.uniform(0.2, np.pi - 0.2),
                          rng.integers(0, 2))
        else:
            v = rng.normal(size=3)
            act[b] = (focus, element, rng.uniform(1.1, 2.1), *(v / np.linalg.norm(v)))
    adv = rng.normal(size=B)
    adv = (adv - adv.mean()) / max(adv.std(), 1e-3)
    data = dict(obs=obs, act=act, logp=rng.normal(-5.0, 1.0, size=B), adv=adv, ret=rng.normal(0.0, 0.3, size=B))
    _check_batch(data, Z, internal)
    return data


def _check_batch(data, Z, internal):
    """the four properties of the module docstring (a batch without them would test nothing new)"""
    ecol = 2 if internal else 1
    obs, el = data['obs'], data['act'][:, ecol].astype(int)
    assert any(l >= 8 for items, _ in obs for l, _ in items)
    assert any(not any(bag[1:8]) and any(c > 0 for c in bag[8:]) for _, bag in obs)
    for want in (8, Z - 1):
        assert any(e == want and bag[want] > 0 for e, (_, bag) in zip(el, obs)), want
    assert any(all(l == 0 for l, _ in items) for items, _ in obs)


def _only_high_bags(Z, N, counts, seed):
    """observations whose bags hold elements of index >= 8 only (four of them, two atoms each: four steps never exhaust one)"""
    rng = np.random.default_rng(seed)
    obs = []
    for b, n in enumerate(counts):
        bag = np.zeros(Z, dtype=np.int64)
        bag[rng.choice(np.arange(8, Z), size=4, replace=False)] = 2
        bag[Z - 1] = 2
        obs.append((_canvas(rng, int(n), N, Z, 8 + (b % (Z - 8))), tuple(int(x) for x in bag)))
    return obs


def _weights(B, seed):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(B, generator=g, dtype=torch.float64) * s for s in (1.0, 0.3, 0.7))


def _backward(out, w):
    wl, we, wv = (x.cuda() for x in w)
    (out['logp'].double() * wl + out['ent'].double() * we + out['v'].double() * wv).sum().backward()
    torch.cuda.synchronize()


def _natoms(obs):
    return [sum(1 for x in o[0] if x[0] != 0) for o in obs]


# ---- 1. CovariantAC against the oracle ------------------------------------------------------------------------------------
COV_CASES = [
    # Z, canvas, atom counts, width, beta ('cfg': the config's -10)
    (9, 6, [6, 0, 1, 5], 128, 'cfg'),     # one past the old arrays; one-launch heads; small-list front kernel
    (13, 6, [6, 0, 1, 5], 128, 'cfg'),    # N = 104: a partial last column tile of the 128-wide GEMM forms
    (16, 6, [6, 0, 1, 5], 128, 'cfg'),    # the cap: N = 128, 4 Z = 64 scalar threads, `small` filled to its seam
    (16, 6, [6, 0, 1, 5], 128, None),     # ... with SO3Distribution instead of ExpSO3Distribution
    (16, 18, [18, 2, 0], 128, 'cfg'),     # canvas above 16: general list build, per-atom kernels ([18, 2] and the empty canvas)
    (16, 6, [6, 0, 1, 5], 256, 'cfg'),    # staged head kernels and row GEMMs
]


@pytest.mark.parametrize('Z,N,counts,width,beta', COV_CASES)
def test_covariant_vs_oracle(built_lib, monkeypatch, Z, N, counts, width, beta):
    # (a seed of its own per case: helpers.oracle_backward caches oracle results by weights, inputs and loss weights -- beta is
    # not part of that key, so two cases that differ in beta alone must not share all three)
    seed = 10 * COV_CASES.index((Z, N, counts, width, beta)) + Z + N
    ac, ref, cfg = _cov_pair(monkeypatch, Z, N, seed=seed, beta=beta, network_width=width)
    data = _batch(Z, N, counts, seed=seed + 1)
    w = _weights(len(counts), seed + 2)
    out = ac.step(data['obs'], data['act'])
    _backward(out, w)
    exp, want = oracle_backward(ref, data, w)
    errs = {k: rel_err(out[k].detach(), exp[k].detach()) for k in ('logp', 'ent', 'v')}
    report = grad_report(ac.theta.grad.detach().double().cpu(), want, ac.slot_table)
    print('outputs', errs, 'worst gradient slot', max((v[0], k) for k, v in report.items() if v[1] >= 1e-10))
    for k in ('logp', 'ent', 'v'):
        assert errs[k] < 1e-5, (k, errs[k])
    assert_grads(report)


def test_covariant_head_outputs_at_16_symbols(built_lib, monkeypatch):
    """mg_cov_head_outputs: the element distribution of step()'s `dists` over 16 symbols against the oracle's"""
    Z, N = 16, 6
    ac, ref, cfg = _cov_pair(monkeypatch, Z, N, seed=41)
    data = _batch(Z, N, [6, 0, 1, 5], seed=42)
    with torch.no_grad():
        out = ac.step(data['obs'], data['act'])
        exp = ref.step(data['obs'], data['act'], dtype=torch.float64, return_internals=True)
    act = torch.as_tensor(data['act'], dtype=torch.float32).cuda()
    element_dist = out['dists'][1]
    assert rel_err(element_dist.log_prob(act[:, 1].round().long()), exp['logps'][1]) < 2e-5   # (as tests/test_gpu_dists.py)
    assert rel_err(element_dist.entropy(), exp['ent_parts'][1], floor=1e-3, abs_tol=1e-7, tol=1e-4) < 1e-4


# ---- 2. SchNetAC against its oracle -----------------------------------------------------------------------------------------
def _int_pair(seed, Z, canvas, width=128):
    from molgym_amd.agents.internal import SchNetAC
    zs = ZS16[:Z]
    torch.manual_seed(seed)
    ac = SchNetAC(ObservationSpace(canvas, zs), ActionSpace(zs), (0.8, 1.8), width, device='cuda:0')
    with torch.no_grad():
        g = torch.Generator().manual_seed(seed + 1)
        for name, (off, shape) in ac.slot_table.items():
            n = int(np.prod(shape))
            if name.endswith('bias'):
                ac.theta[off:off + n] = (0.1 * torch.randn(n, generator=g)).to(ac.theta)
    ref = SchNetACRef(zs, canvas, (0.8, 1.8), width).double()
    ref.load_state_dict({k: v.double().cpu() for k, v in ac.export_state_dict().items()}, strict=True)
    return ac, ref


@pytest.mark.parametrize('Z,N,counts', [(9, 6, [6, 0, 1, 5]), (16, 6, [6, 0, 1, 5]), (16, 20, [20, 17, 0, 3])])
def test_schnet_vs_oracle(built_lib, Z, N, counts):
    """canvas 6: the one-launch heads (above eight symbols the plain walk, k_int_heads_fwd / _bwd); canvas 20: the grouped-GEMM
    heads.  Tolerances of tests/test_gpu_wide_canvas.py::test_schnet_vs_oracle."""
    ac, ref = _int_pair(Z + N, Z, N)
    data = _batch(Z, N, counts, seed=Z + N + 3, internal=True)
    w = _weights(len(counts), Z + N + 4)
    out = ac.step(data['obs'], data['act'])
    _backward(out, w)
    exp = ref.step(data['obs'], data['act'], dtype=torch.float64)
    (exp['logp'] * w[0] + exp['ent'] * w[1] + exp['v'] * w[2]).sum().backward()
    errs = {k: rel_err(out[k], exp[k]) for k in ('logp', 'ent', 'v')}
    got = ac.theta.grad.double().cpu()
    want = dict(ref.named_parameters())
    bad, worst = {}, (0.0, '')
    for name, (off, shape) in ac.slot_table.items():
        n = int(np.prod(shape))
        gw = want[name].grad
        gw = torch.zeros(n, dtype=torch.float64) if gw is None else gw.reshape(-1)
        scale = gw.abs().max().item()
        err = (got[off:off + n] - gw).abs().max().item() / max(scale, 1e-12)
        if scale >= 1e-10:
            worst = max(worst, (err, name))
        if not (err < 2e-4 or scale < 1e-10):
            bad[name] = (err, scale)
    print('outputs', errs, 'worst gradient slot', worst)
    for k in ('logp', 'ent', 'v'):
        assert errs[k] < 1e-5, (k, errs[k])
    assert not bad, bad


# ---- 3. PPO step ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('graph', [True, False], ids=['graph', 'stream'])
def test_covariant_ppo_step_at_16_symbols(built_lib, monkeypatch, graph):
    """the one-call PPO mini-batch == compute_loss + autograd (assertions of test_covariant_ppo_step_at_canvas_96)"""
    from molgym_amd import ppo as hip_ppo
    ac, ref, cfg = _cov_pair(monkeypatch, 16, 6, seed=7)
    data = _batch(16, 6, [6, 0, 1, 5, 3, 2, 6, 4], seed=8)
    batch = ac.prepare_batch(data['obs'], data['act'], data['logp'], data['adv'], data['ret'])
    ac.theta.grad = torch.zeros_like(ac.theta)
    ac.ppo_minibatch(batch, 0.2, 0.5, 0.01, graph=graph)
    torch.cuda.synchronize()
    assert ac.last_step_used_graph == graph
    g_dev = ac.theta.grad.clone()
    ac.theta.grad = None
    loss, _ = hip_ppo.compute_loss(ac, data, 0.2, 0.5, 0.01)
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(g_dev).all()
    assert (g_dev - ac.theta.grad).abs().max().item() <= 2e-4 * ac.theta.grad.abs().max().item()


@pytest.mark.parametrize('graph', [True, False], ids=['graph', 'stream'])
def test_schnet_ppo_step_at_16_symbols(built_lib, graph):
    """assertions of test_schnet_ppo_step_at_canvas_128"""
    from molgym_amd import ppo
    ac, _ = _int_pair(21, 16, 20)
    data = _batch(16, 20, [20, 0, 17, 3, 1, 12, 20, 7], seed=22, internal=True)
    loss, info = ppo.compute_loss(ac, data, clip_ratio=0.2, vf_coef=0.5, entropy_coef=0.01)
    ac.theta.grad = None
    loss.backward()
    want = ac.theta.grad.clone()
    ac.theta.grad = None
    stats = ac.ppo_minibatch(ac.prepare_batch(data['obs'], data['act'], data['logp'], data['adv'], data['ret']), 0.2, 0.5, 0.01,
                             graph=graph)
    torch.cuda.synchronize()
    assert (ac.theta.grad - want).abs().max().item() < 1e-5 * want.abs().max().item()
    assert abs(stats[0].item() - info['policy_loss']) < 1e-6 * max(1.0, abs(info['policy_loss']))


# ---- 4. sampling ------------------------------------------------------------------------------------------------------------
def test_covariant_sampling_at_16_symbols(built_lib, monkeypatch):
    Z, N = 16, 6
    ac, ref, cfg = _cov_pair(monkeypatch, Z, N, seed=9)
    data = _batch(Z, N, [6, 0, 1, 5, 3, 4], seed=10)
    obs = data['obs']
    bags = np.array([bag for _, bag in obs])
    assert not bags[0, :8].any()   # sample 0 may only choose among the indices >= 8
    # evaluation: the drawn element is the arg-max of the oracle's element logits (given the drawn focus) over the elements the
    # bag holds; two logits closer than 1e-5 count as a tie (float32 against float64)
    ac.training = False
    with torch.no_grad():
        a = ac.step(obs)['a'].cpu().numpy()
        exp = ref.step(obs, a.astype(np.float64), dtype=torch.float64, return_internals=True)
    logits = exp['element_logits'].numpy()
    masked = np.where(bags > 0, logits, -np.inf)
    drawn = a[:, 1].astype(int)
    assert np.all(bags[np.arange(len(obs)), drawn] > 0)
    assert drawn[0] >= 8
    assert np.all(masked[np.arange(len(obs)), drawn] >= masked.max(axis=1) - 1e-5), (drawn, masked.argmax(axis=1))
    # training: element frequencies of one observation (a single atom: the focus is always 0, so the element distribution is
    # one masked softmax) repeated 512 times over 8 seeds, with the bound of the focus test of tests/test_gpu_wide_canvas.py
    ob = obs[2]
    assert _natoms([ob]) == [1]
    bag = np.array(ob[1])
    with torch.no_grad():
        one = ref.step([ob], np.array([[0, int(np.nonzero(bag)[0][0]), 1.3, 0.0, 0.6, 0.8]]), dtype=torch.float64, return_internals=True)
    lg = torch.where(torch.from_numpy(bag > 0), one['element_logits'][0], torch.tensor(-float('inf'), dtype=torch.float64))
    p_el = torch.softmax(lg, dim=0).numpy()
    ac.training = True
    draws = []
    with torch.no_grad():
        for s in range(8):
            torch.manual_seed(100 + s)
            draws.append(ac.step([ob] * 512)['a'][:, 1].cpu().numpy())
    e = np.concatenate(draws).astype(int)
    assert e.min() >= 0 and e.max() < Z
    freq = np.bincount(e, minlength=Z)[:Z] / len(e)
    assert np.abs(freq - p_el).max() < 4 * np.sqrt(0.25 / len(e)) + 1e-3, (freq, p_el)
    assert np.all(freq[bag == 0] == 0)


def _schnet_element_logits(ref, obs, a):
    """the oracle's element logits given the focus column of the action rows `a` (internal_ref.py:163-193 up to phi_element)"""
    dt = torch.float64
    rows = []
    with torch.no_grad():
        for (atoms, bag), row in zip([ref._atoms(o) for o in obs], a):
            lbag = ref.phi_beta(torch.tensor(bag, dtype=dt)[None])[0]
            f = int(round(float(row[1])))
            feat = torch.zeros(ref.num_afeats, dtype=dt)
            if len(atoms):
                feat = ref._embed([z for z, _ in atoms], [p for _, p in atoms], dt)[f]
            rows.append(ref.phi_element(torch.cat([feat, lbag])[None])[0])
    return torch.stack(rows).numpy()


def test_schnet_evaluation_picks_the_masked_argmax_element(built_lib):
    """tie rule of test_schnet_step_canvas_evaluation_at_canvas_96: logits closer than 1e-5 count as equal"""
    Z, N = 16, 6
    ac, ref = _int_pair(23, Z, N)
    ac.training = False
    obs = _batch(Z, N, [6, 0, 1, 5, 3, 4], seed=24, internal=True)['obs']
    with torch.no_grad():
        a = ac.step(obs)['a'].cpu().numpy()
    bags = np.array([bag for _, bag in obs])
    masked = np.where(bags > 0, _schnet_element_logits(ref, obs, a), -np.inf)
    drawn = a[:, 2].astype(int)
    assert drawn[0] >= 8
    assert np.all(bags[np.arange(len(obs)), drawn] > 0)
    assert np.all(masked[np.arange(len(obs)), drawn] >= masked.max(axis=1) - 1e-5), (drawn, masked.argmax(axis=1))


# ---- 5. device canvases -------------------------------------------------------------------------------------------------------
def _canvas_steps(ac, zs, N, obs):
    """four committed steps; after each the device canvas equals a parse of the observations with the returned atoms appended
    (the loop of test_covariant_step_canvas_across_64_atoms).  A truncated symbol table places a charge of 0."""
    canvas = ac.make_canvas(obs)
    assert canvas.matches(obs)
    placed, start = 0, _natoms(obs)
    for it in range(4):
        natoms = _natoms(obs)
        torch.manual_seed(200 + it)
        with torch.no_grad():
            got = ac.step_canvas(canvas)
        nxt = []
        for (items, bag), n, (e, p) in zip(obs, natoms, got['actions']):
            items, bag = list(items), list(bag)
            assert e >= 8 and bag[e] > 0, (e, bag)
            if zs[e] != 0 and n < N:
                items[n] = (e, tuple(float(x) for x in p))
                bag[e] -= 1
                placed += 1
            nxt.append((tuple(items), tuple(bag)))
        obs = nxt
        assert canvas.matches(obs), it
    assert placed == 4 * len(obs) and _natoms(obs) == [n + 4 for n in start]


def test_covariant_step_canvas_at_16_symbols(built_lib, monkeypatch):
    ac, ref, cfg = _cov_pair(monkeypatch, 16, 8, seed=11)
    _canvas_steps(ac, ZS16, 8, _only_high_bags(16, 8, [3, 0, 1, 4, 2, 0, 4, 1], seed=12))


def test_schnet_step_canvas_at_16_symbols(built_lib):
    ac, _ = _int_pair(25, 16, 8)
    ac.training = True
    _canvas_steps(ac, ZS16, 8, _only_high_bags(16, 8, [3, 0, 1, 4, 2, 0, 4, 1], seed=26))


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------
def test_17_symbols_are_refused_at_construction(built_lib, monkeypatch):
    from molgym_amd.agents.internal import SchNetAC
    zs = ZS16 + [85]
    monkeypatch.setitem(CONFIGS, 'zs17', dict(zs=zs, canvas_size=6, batch=16, bag_scale=20, beta=-10.0))
    with pytest.raises(RuntimeError, match='16'):
        make_pair('zs17', seed=0)
    with pytest.raises(RuntimeError, match='16'):
        SchNetAC(ObservationSpace(6, zs), ActionSpace(zs), (0.8, 1.8), 128, device='cuda:0')


def test_product_limit_is_refused_without_a_build(built_lib, monkeypatch):
    """13 symbols x 5 channels per element = 65 > 64: refused before the (10, 5) library is looked for or compiled"""
    monkeypatch.setitem(CONFIGS, 'zs13', dict(zs=ZS16[:13], canvas_size=6, batch=16, bag_scale=20, beta=-10.0))
    built = []
    monkeypatch.setattr(_lib, 'build_variant', lambda *a, **k: built.append(a))
    with pytest.raises(RuntimeError, match=r'num_channels_per_element.*64'):
        make_pair('zs13', seed=0, num_channels_per_element=5)
    assert not built


def test_library_refuses_17_symbols(built_lib, monkeypatch):
    ac, _, _ = _cov_pair(monkeypatch, 16, 6, seed=1)
    nbytes = C.c_size_t()
    cfg = ac._make_cfg(4, np.full(4, 6))
    assert built_lib.mg_cov_workspace_bytes(C.byref(cfg), C.byref(nbytes)) == 0
    cfg.Z = 17
    assert built_lib.mg_cov_workspace_bytes(C.byref(cfg), C.byref(nbytes)) != 0
    assert '16' in built_lib.mg_last_error().decode()
    iac, _ = _int_pair(2, 16, 6)
    icfg = iac._canvas_cfg(np.full(4, 6))
    assert built_lib.mg_int_workspace_bytes(C.byref(icfg), C.byref(nbytes)) == 0
    icfg.Z = 17
    assert built_lib.mg_int_workspace_bytes(C.byref(icfg), C.byref(nbytes)) != 0
    assert '16' in built_lib.mg_last_error().decode()
