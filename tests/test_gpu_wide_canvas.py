"""Canvases above 64 atoms (up to MG_MAX_CANVAS = 255) in both agents: CovariantAC's staged heads and SchNetAC's head kernels
with K focus logits per lane, against the float64 oracles; the PPO step, sampling and device canvases past 64 atoms; and the
refusals of what the kernels cannot address."""
import ctypes as C

import numpy as np
import pytest
import torch

from molgym_amd import _lib
from molgym_amd.spaces import ActionSpace, ObservationSpace
from molgym_amd.synthetic import CONFIGS, MODEL_DEFAULTS
from oracle.covariant_ref import CovariantACRef
from oracle.internal_ref import SchNetACRef
from tests.helpers import assert_grads, grad_report, make_pair, oracle_backward, rel_err

pytestmark = pytest.mark.gpu
ZS = [0, 1, 6, 7, 8]


def _cov_pair(monkeypatch, N, seed):
    """make_pair on a canvas of N atoms (cfg5's elements, bag scale and beta)"""
    name = f'wide{N}'
    monkeypatch.setitem(CONFIGS, name, dict(zs=ZS, canvas_size=N, batch=16, bag_scale=20, beta=-10.0))
    return make_pair(name, seed=seed)


def _canvas(rng, n, N):
    """synthetic.make_canvas's random walk (bonds U(1.10, 2.10), no pair closer than 0.6), the distance test vectorised"""
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
    labels = rng.integers(1, len(ZS), size=n)
    return tuple([(int(l), tuple(float(x) for x in p)) for l, p in zip(labels, pos[:n])] + [(0, (0.0, 0.0, 0.0))] * (N - n))


def _batch(N, counts, seed, internal=False):
    """observations with the given atom counts, valid actions (covariant: 6 columns; SchNetAC: 7) and PPO loss inputs; the
    focus of every other sample is its last atom (lanes past 64 pick)"""
    rng = np.random.default_rng(seed)
    B = len(counts)
    obs = []
    act = np.zeros((B, 7 if internal else 6))
    for b, n in enumerate(counts):
        bag = rng.integers(1, 4, size=len(ZS))
        bag[0] = 0
        obs.append((_canvas(rng, int(n), N), tuple(int(x) for x in bag)))
        focus = max(int(n) - 1, 0) if b % 2 else rng.integers(0, max(int(n), 1))
        element = rng.integers(1, len(ZS))
        if internal:
            act[b, 1:] = (focus, element, rng.uniform(1.1, 2.1), rng.uniform(0.3, np.pi - 0.3), rng.uniform(0.2, np.pi - 0.2),
                          rng.integers(0, 2))
        else:
            v = rng.normal(size=3)
            act[b] = (focus, element, rng.uniform(1.1, 2.1), *(v / np.linalg.norm(v)))
    adv = rng.normal(size=B)
    adv = (adv - adv.mean()) / max(adv.std(), 1e-3)
    return dict(obs=obs, act=act, logp=rng.normal(-5.0, 1.0, size=B), adv=adv, ret=rng.normal(0.0, 0.3, size=B))


def _weights(B, seed):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(B, generator=g, dtype=torch.float64) * s for s in (1.0, 0.3, 0.7))


def _backward(out, w):
    wl, we, wv = (x.cuda() for x in w)
    (out['logp'].double() * wl + out['ent'].double() * we + out['v'].double() * wv).sum().backward()
    torch.cuda.synchronize()


# ---- CovariantAC --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,counts', [(64, [64]), (65, [0, 64, 65]), (128, [128, 3]), (255, [255, 0])])
def test_covariant_vs_oracle(built_lib, monkeypatch, N, counts):
    """canvas 64: the old boundary (one-launch heads); 65 and up: the staged heads, a canvas of 65 atoms on both sides of the
    64-lane boundary, and empty canvases (the lone zero focus logit)"""
    ac, ref, cfg = _cov_pair(monkeypatch, N, seed=N)
    data = _batch(N, counts, seed=N + 1)
    w = _weights(len(counts), N + 2)
    out = ac.step(data['obs'], data['act'])
    _backward(out, w)
    exp, want = oracle_backward(ref, data, w)
    for k in ('logp', 'ent', 'v'):
        assert rel_err(out[k].detach(), exp[k].detach()) < 1e-5, (k, rel_err(out[k].detach(), exp[k].detach()))
    assert_grads(grad_report(ac.theta.grad.detach().double().cpu(), want, ac.slot_table))


def test_covariant_full_minibatch_at_canvas_255(built_lib, monkeypatch):
    """140 nearly full 255-atom canvases (9 M edges): the whole batch runs with the output adjoint zero outside two small
    samples, which the oracle evaluates on their own (as tests/test_gpu_large.py); then every sample of the batch against the
    same sample evaluated alone"""
    N, B = 255, 140
    ac, ref, cfg = _cov_pair(monkeypatch, N, seed=3)
    rng = np.random.default_rng(4)
    counts = rng.integers(240, N + 1, size=B)
    counts[0] = N
    pick = np.array([17, 101])
    counts[pick] = (40, 64)
    data = _batch(N, counts, seed=5)
    w2 = _weights(2, 6)
    w = torch.zeros(3, B, dtype=torch.float64)
    for r in range(3):
        w[r, torch.from_numpy(pick)] = w2[r]
    out = ac.step(data['obs'], data['act'])
    _backward(out, tuple(w))
    # the dense oracle pays for every slot of the canvas: the two samples go to a copy built for 64 slots (same weights; their
    # atoms fill the first slots, the rest are padding either way)
    ref64 = CovariantACRef(zs=ZS, canvas_size=64, bag_scale=cfg['bag_scale'], beta=cfg['beta'], **MODEL_DEFAULTS).double()
    ref64.load_state_dict(ref.state_dict())
    sub = dict(obs=[(data['obs'][i][0][:64], data['obs'][i][1]) for i in pick], act=data['act'][pick])
    exp, want = oracle_backward(ref64, sub, w2)
    for k in ('logp', 'ent', 'v'):
        got = out[k].detach().cpu()[torch.from_numpy(pick)]
        assert rel_err(got, exp[k].detach()) < 1e-5, (k, rel_err(got, exp[k].detach()))
    assert_grads(grad_report(ac.theta.grad.detach().double().cpu(), want, ac.slot_table))
    with torch.no_grad():
        alone = [ac.step([data['obs'][b]], data['act'][b:b + 1]) for b in range(B)]
    for k in ('logp', 'ent', 'v'):
        one = torch.cat([a[k].detach().cpu() for a in alone])
        assert rel_err(out[k].detach().cpu(), one) < 1e-5, (k, rel_err(out[k].detach().cpu(), one))


def test_covariant_ppo_step_at_canvas_96(built_lib, monkeypatch):
    """the one-call PPO mini-batch (graph launch) with the staged heads == compute_loss + autograd"""
    from molgym_amd import ppo as hip_ppo
    ac, ref, cfg = _cov_pair(monkeypatch, 96, seed=7)
    data = _batch(96, [96, 0, 65, 64, 90, 12, 70, 33], seed=8)
    batch = ac.prepare_batch(data['obs'], data['act'], data['logp'], data['adv'], data['ret'])
    ac.theta.grad = torch.zeros_like(ac.theta)
    ac.ppo_minibatch(batch, 0.2, 0.5, 0.01)
    torch.cuda.synchronize()
    g_dev = ac.theta.grad.clone()
    ac.theta.grad = None
    loss, _ = hip_ppo.compute_loss(ac, data, 0.2, 0.5, 0.01)
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(g_dev).all()
    assert (g_dev - ac.theta.grad).abs().max().item() <= 2e-4 * ac.theta.grad.abs().max().item()


def test_covariant_sampling_at_canvas_96(built_lib, monkeypatch):
    ac, ref, cfg = _cov_pair(monkeypatch, 96, seed=9)
    data = _batch(96, [96, 80, 70, 65, 30, 0], seed=10)
    big = [0, 1, 2, 3]  # n > 64
    with torch.no_grad():
        exp = ref.step([data['obs'][i] for i in big], data['act'][big], dtype=torch.float64, return_internals=True)
    # evaluation: the arg-max focus
    ac.training = False
    with torch.no_grad():
        a = ac.step(data['obs'])['a'].cpu().numpy()
    for r, i in enumerate(big):
        n = sum(1 for it in data['obs'][i][0] if it[0] != 0)
        assert int(a[i, 0]) == int(torch.argmax(exp['focus_logits'][r, :n])), i
    # training: focus frequencies of one 70-atom observation follow the oracle's probabilities
    ob = data['obs'][2]
    n = 70
    p_focus = torch.softmax(exp['focus_logits'][2, :n], dim=0).numpy()
    ac.training = True
    draws = []
    with torch.no_grad():
        for s in range(8):
            torch.manual_seed(100 + s)
            draws.append(ac.step([ob] * 512)['a'][:, 0].cpu().numpy())
    f = np.concatenate(draws).astype(int)
    assert f.min() >= 0 and f.max() < n
    freq = np.bincount(f, minlength=n)[:n] / len(f)
    assert np.abs(freq - p_focus).max() < 4 * np.sqrt(0.25 / len(f)) + 1e-3, (freq, p_focus)
    # every drawn focus is one of the sample's atoms
    with torch.no_grad():
        a = ac.step(data['obs'] * 16)['a'].cpu().numpy()
    natoms = np.array([sum(1 for it in o[0] if it[0] != 0) for o in data['obs'] * 16])
    assert np.all(a[:, 0] < np.maximum(natoms, 1))


def test_covariant_step_canvas_across_64_atoms(built_lib, monkeypatch):
    """committed steps take canvases of 62 - 64 atoms past 64: after each step the device canvas equals a parse of the
    observations with the returned atoms appended"""
    N = 72
    ac, ref, cfg = _cov_pair(monkeypatch, N, seed=11)
    obs = _batch(N, [62, 63, 64, 64, 63, 62, 64, 63], seed=12)['obs']
    canvas = ac.make_canvas(obs)
    assert canvas.matches(obs)
    for it in range(4):
        natoms = [sum(1 for x in o[0] if x[0] != 0) for o in obs]
        torch.manual_seed(200 + it)
        with torch.no_grad():
            got = ac.step_canvas(canvas)
        a = got['a'].cpu().numpy()
        assert np.all(a[:, 0] < np.maximum(natoms, 1))
        nxt = []
        for (items, bag), n, (e, p) in zip(obs, natoms, got['actions']):
            items, bag = list(items), list(bag)
            if ZS[e] != 0 and n < N:
                items[n] = (e, p)
                bag[e] -= 1
            nxt.append((tuple(items), tuple(bag)))
        obs = nxt
        assert canvas.matches(obs), it
    assert min(sum(1 for x in o[0] if x[0] != 0) for o in obs) > 64


# ---- SchNetAC -----------------------------------------------------------------------------------------------------------
def _int_pair(seed, canvas, width=128):
    from molgym_amd.agents.internal import SchNetAC
    torch.manual_seed(seed)
    ac = SchNetAC(ObservationSpace(canvas, ZS), ActionSpace(ZS), (0.8, 1.8), width, device='cuda:0')
    with torch.no_grad():
        g = torch.Generator().manual_seed(seed + 1)
        for name, (off, shape) in ac.slot_table.items():
            n = int(np.prod(shape))
            if name.endswith('bias'):
                ac.theta[off:off + n] = (0.1 * torch.randn(n, generator=g)).to(ac.theta)
    ref = SchNetACRef(ZS, canvas, (0.8, 1.8), width).double()
    ref.load_state_dict({k: v.double().cpu() for k, v in ac.export_state_dict().items()}, strict=True)
    return ac, ref


@pytest.mark.parametrize('N', [63, 64, 128, 255])
def test_schnet_vs_oracle(built_lib, N):
    """63: one focus logit per lane (the form every canvas up to 63 runs); 64: the first canvas with two per lane (molecules of
    65 atoms); 128: two; 255: four"""
    ac, ref = _int_pair(N, N)
    counts = [N, N - 1, 65 if N >= 65 else 5, 0, 3]
    data = _batch(N, counts, seed=N + 3, internal=True)
    w = _weights(len(counts), N + 4)
    out = ac.step(data['obs'], data['act'])
    _backward(out, w)
    exp = ref.step(data['obs'], data['act'], dtype=torch.float64)
    (exp['logp'] * w[0] + exp['ent'] * w[1] + exp['v'] * w[2]).sum().backward()
    for k in ('logp', 'ent', 'v'):
        assert rel_err(out[k], exp[k]) < 1e-5, (k, rel_err(out[k], exp[k]))
    got = ac.theta.grad.double().cpu()
    want = dict(ref.named_parameters())
    bad = {}
    for name, (off, shape) in ac.slot_table.items():
        n = int(np.prod(shape))
        gw = want[name].grad
        gw = torch.zeros(n, dtype=torch.float64) if gw is None else gw.reshape(-1)
        scale = gw.abs().max().item()
        err = (got[off:off + n] - gw).abs().max().item() / max(scale, 1e-12)
        if not (err < 2e-4 or scale < 1e-10):
            bad[name] = (err, scale)
    assert not bad, bad


def test_schnet_ppo_step_at_canvas_128(built_lib):
    from molgym_amd import ppo
    ac, _ = _int_pair(21, 128)
    data = _batch(128, [128, 100, 64, 0, 70, 127, 5, 90], seed=22, internal=True)
    loss, info = ppo.compute_loss(ac, data, clip_ratio=0.2, vf_coef=0.5, entropy_coef=0.01)
    ac.theta.grad = None
    loss.backward()
    want = ac.theta.grad.clone()
    ac.theta.grad = None
    stats = ac.ppo_minibatch(ac.prepare_batch(data['obs'], data['act'], data['logp'], data['adv'], data['ret']), 0.2, 0.5, 0.01)
    torch.cuda.synchronize()
    assert (ac.theta.grad - want).abs().max().item() < 1e-5 * want.abs().max().item()
    assert abs(stats[0].item() - info['policy_loss']) < 1e-6 * max(1.0, abs(info['policy_loss']))


def test_schnet_step_canvas_evaluation_at_canvas_96(built_lib):
    ac, _ = _int_pair(23, 96)
    ac.training = False
    obs = _batch(96, [96, 95, 80, 64, 63, 0, 1, 2, 70, 30], seed=24, internal=True)['obs']
    cv = ac.make_canvas(obs)
    with torch.no_grad():
        got = ac.step_canvas(cv, commit=False)
        kv = ac._ws_view(ac._last_sample_cfg, ac._last_ws, 'kv')[:2 * len(obs)].view(2, -1).t().cpu().numpy()
        want = ac.step(obs)
    assert cv.matches(obs)
    ga, wa = got['a'].cpu().numpy(), want['a'].cpu().numpy()
    assert np.array_equal(ga[:, :3], wa[:, :3])
    assert np.abs(ga[:, 3:6] - wa[:, 3:6]).max() <= 1e-6
    same = ga[:, 6] == wa[:, 6]
    assert np.all(same | (np.abs(kv[:, 0] - kv[:, 1]) < 1e-5))
    rows = np.nonzero(same)[0]
    for k in ('logp', 'ent', 'v'):
        assert rel_err(got[k][rows], want[k][rows]) < 1e-5, k


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_canvas_256_is_refused_at_construction(built_lib, monkeypatch):
    from molgym_amd.agents.internal import SchNetAC
    with pytest.raises(RuntimeError, match='255'):
        _cov_pair(monkeypatch, 256, seed=0)
    with pytest.raises(RuntimeError, match='255'):
        SchNetAC(ObservationSpace(256, ZS), ActionSpace(ZS), (0.8, 1.8), 128, device='cuda:0')


def test_shapes_past_the_per_edge_limit_are_refused(built_lib, monkeypatch):
    """the workspace query (host only: what both agents call before any launch) refuses a mini-batch whose per-edge matrices
    pass 2^31 elements, naming B and the canvas size; 140 full 255-atom canvases (covariant) / 85 (SchNetAC) are accepted"""
    lib = _lib.lib()
    ac, _, _ = _cov_pair(monkeypatch, 255, seed=1)
    nbytes = C.c_size_t()
    cfg = ac._make_cfg(140, np.full(140, 255))
    assert lib.mg_cov_workspace_bytes(C.byref(cfg), C.byref(nbytes)) == 0
    cfg = ac._make_cfg(240, np.full(240, 255))
    assert lib.mg_cov_workspace_bytes(C.byref(cfg), C.byref(nbytes)) != 0
    msg = lib.mg_last_error().decode()
    assert 'B=240' in msg and 'canvas_size 255' in msg, msg
    cfg.N = 256
    assert lib.mg_cov_workspace_bytes(C.byref(cfg), C.byref(nbytes)) != 0
    assert '255' in lib.mg_last_error().decode()
    iac, _ = _int_pair(2, 255)
    cfg = iac._canvas_cfg(np.full(85, 255))
    assert lib.mg_int_workspace_bytes(C.byref(cfg), C.byref(nbytes)) == 0
    cfg = iac._canvas_cfg(np.full(86, 255))
    assert lib.mg_int_workspace_bytes(C.byref(cfg), C.byref(nbytes)) != 0
    msg = lib.mg_last_error().decode()
    assert 'B=86' in msg and 'canvas_size 255' in msg, msg
