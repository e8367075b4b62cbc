"""Deterministic mode (molgym_amd.set_deterministic) on SchNetAC: the backward, the PPO mini-batch step, the gradient norm and
ppo.train give the same bits on every run and however the step is issued -- where tests/test_gpu_internal.py has to allow the
2e-5 of the default mode's float atomics, these are torch.equal.

Cases (canvas, width, B): (7, 128, 33) one-launch heads and fused interactions; (7, 64, 20) plain-walk heads; (20, 128, 9) molecules
above 16 atoms (grouped GEMM heads, per-layer interactions); (3, 128, 12) with empty, one- and two-atom canvases (masks)."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from molgym_amd.spaces import ActionSpace, ObservationSpace
from molgym_amd.synthetic import make_batch_internal
from oracle.internal_ref import SchNetACRef
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu
ZS = [0, 9, 16]
CASES = [(7, 128, 33), (7, 64, 20), (20, 128, 9), (3, 128, 12)]
HP = (0.2, 0.5, 0.01)


@pytest.fixture(autouse=True)
def _restore_switch(built_lib):
    from molgym_amd import _lib
    prev = _lib.is_deterministic()
    yield
    _lib.set_deterministic(prev)


def _agent(seed, width, canvas, with_ref=False):
    from molgym_amd.agents.internal import SchNetAC
    torch.manual_seed(seed)
    ac = SchNetAC(ObservationSpace(canvas, ZS), ActionSpace(ZS), (0.8, 1.8), width, device='cuda:0')
    with torch.no_grad():
        g = torch.Generator().manual_seed(seed + 1)
        for name, (off, shape) in ac.slot_table.items():
            n = int(np.prod(shape))
            if name.endswith('bias'):
                ac.theta[off:off + n] = (0.1 * torch.randn(n, generator=g)).to(ac.theta)
    if not with_ref:
        return ac
    ref = SchNetACRef(ZS, canvas, (0.8, 1.8), width).double()
    ref.load_state_dict({k: v.double().cpu() for k, v in ac.export_state_dict().items()}, strict=True)
    return ac, ref


def _data(canvas, B, seed):
    """make_batch_internal; the canvas-3 case gets an empty, a one-atom and a two-atom canvas (focus 0), as
    tests/test_gpu_internal.py::test_small_canvases_and_masks builds them.

    No canvas of that case is full: make_batch also draws canvases of three atoms out of three, which no agent ever acts on, and
    they are the only samples of the case whose kappa term counts (n >= 3).  With exactly three atoms the two dihedral signs are
    mirror images in the plane of those atoms, every distance is the same, and phi_kappa's gradient is the difference of two equal
    embeddings: exactly zero, but 2e-9 of rounding in the float64 oracle (above the 1e-10 below which the bound of
    test_outputs_and_gradients_match_oracle takes a gradient for zero) and 1e-7 in the float32 forward that both modes share.  Kappa terms that
    count are in the other three cases; here the last atom of such a canvas is removed, so the case is the masks alone."""
    d = make_batch_internal(B, canvas, ZS, seed=seed)
    if canvas == 3:
        empty = (0, (0.0, 0.0, 0.0))
        obs = list(d['obs'])
        full = max(obs, key=lambda o: sum(1 for it in o[0] if ZS[it[0]] != 0))
        for b, keep in enumerate((0, 1, 2)):
            cv = tuple(item if i < keep else empty for i, item in enumerate(full[0]))
            obs[b] = (cv, full[1])
            d['act'][b, 1] = 0
        for b in range(3, len(obs)):
            if all(ZS[it[0]] != 0 for it in obs[b][0]):
                obs[b] = (obs[b][0][:-1] + (empty, ), obs[b][1])
                d['act'][b, 1] = min(d['act'][b, 1], canvas - 2)
        d['obs'] = obs
    return d


def _batch(ac, d):
    return ac.prepare_batch(d['obs'], d['act'], d['logp'], d['adv'], d['ret'])


def _step_grad(ac, batch, **kw):
    ac.theta.grad = torch.zeros_like(ac.theta)
    stats = ac.ppo_minibatch(batch, *HP, **kw)
    torch.cuda.synchronize()
    return stats.clone(), ac.theta.grad.clone()


@pytest.mark.parametrize('canvas,width,B', CASES)
def test_same_bits_on_every_run_and_in_every_form(built_lib, canvas, width, B):
    import molgym_amd
    molgym_amd.set_deterministic(True)
    ac = _agent(2, width, canvas)
    batch = _batch(ac, _data(canvas, B, seed=10))
    # three runs from a zeroed gradient
    s0, g0 = _step_grad(ac, batch, graph=False)
    assert torch.isfinite(g0).all() and g0.abs().max().item() > 0
    for _ in range(2):
        s, g = _step_grad(ac, batch, graph=False)
        assert torch.equal(s, s0) and torch.equal(g, g0)
    # graph form == stream form (a deterministic step is issued as stream launches either way)
    s, g = _step_grad(ac, batch, graph=True)
    assert torch.equal(s, s0) and torch.equal(g, g0)
    # epoch cache on / off over five ragged mini-batches through one cached workspace
    batches = [_batch(ac, _data(canvas, n, seed=40 + k)) for k, n in enumerate((B, max(B - 7, 1), 3, B + 5, B))]
    res = {}
    for cached in (False, True):
        ac.theta.grad = torch.zeros_like(ac.theta)
        ac.invalidate_weights()
        acc = torch.zeros(6, dtype=torch.float64, device='cuda')
        outs = [ac.ppo_minibatch(b, *HP, loss_scale=0.5, stats_accum=acc, epoch_cache=cached).clone() for b in batches]
        if cached:
            ac.fold_gradients()
        torch.cuda.synchronize()
        res[cached] = (outs, ac.theta.grad.clone(), acc.clone())
    for a, b in zip(res[False][0], res[True][0]):
        assert torch.equal(a, b)
    assert torch.equal(res[False][1], res[True][1]) and torch.equal(res[False][2], res[True][2])


@pytest.mark.parametrize('canvas,width,B', CASES)
def test_parity_with_the_oracle_and_the_default_mode(built_lib, canvas, width, B):
    """bounds of tests/test_gpu_internal.py::test_outputs_and_gradients_match_oracle"""
    import molgym_amd
    ac, ref = _agent(0, width, canvas, with_ref=True)
    data = _data(canvas, B, seed=4)
    g = torch.Generator().manual_seed(1)
    wl, we, wv = (torch.randn(B, generator=g, dtype=torch.float64) * s for s in (1.0, 0.3, 0.7))
    exp = ref.step(data['obs'], data['act'], dtype=torch.float64)
    (exp['logp'] * wl + exp['ent'] * we + exp['v'] * wv).sum().backward()
    batch = _batch(ac, data)
    res = {}
    for det in (False, True):
        molgym_amd.set_deterministic(det)
        ac.theta.grad = None
        out = ac.step(data['obs'], data['act'])
        (out['logp'].double() * wl.cuda() + out['ent'].double() * we.cuda() + out['v'].double() * wv.cuda()).sum().backward()
        torch.cuda.synchronize()
        res[det] = ({k: out[k].detach().clone() for k in ('logp', 'ent', 'v')}, ac.theta.grad.clone(), _step_grad(ac, batch))
    out, grad = res[True][0], res[True][1]
    tol = 2e-5 if width == 64 else 1e-5
    for k in ('logp', 'ent', 'v'):
        print(k, rel_err(out[k], exp[k]))
        assert rel_err(out[k], exp[k]) < tol, (k, rel_err(out[k], exp[k]))
    got = grad.double().cpu()
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
    # against the default mode: outputs and statistics bit for bit, gradients within the default mode's own 2e-5
    for k in ('logp', 'ent', 'v'):
        assert torch.equal(res[False][0][k], res[True][0][k]), k
    assert torch.equal(res[False][2][0], res[True][2][0])
    for g0, g1 in ((res[False][1], res[True][1]), (res[False][2][1], res[True][2][1])):
        d = (g0 - g1).abs().max().item()
        print('default vs deterministic', d, g0.abs().max().item())
        assert d <= 2e-5 * g0.abs().max().item()


@pytest.mark.parametrize('canvas,width,B', CASES)
def test_autograd_path_equals_the_fused_step(built_lib, canvas, width, B):
    """step(obs, actions) + backward() == ppo_minibatch at loss_scale 1, bit for bit.  The two paths meet at gout = d loss / d (logp,
    ent, v): the fused step forms it in the loss kernel, so the autograd path is fed the same kernel's result (mg_ppo_loss on the
    outputs of step()) -- torch's own float64 autograd of compute_loss rounds that seam differently, which is not what is under test"""
    import molgym_amd
    from molgym_amd import _lib
    molgym_amd.set_deterministic(True)
    ac = _agent(14, width, canvas)
    data = _data(canvas, B, seed=31)
    batch = _batch(ac, data)
    stats, want = _step_grad(ac, batch)
    ac.theta.grad = None
    out = ac.step(data['obs'], data['act'])
    pred = torch.stack([out['logp'], out['ent'], out['v']]).detach().contiguous()
    gout = torch.empty(3, B, dtype=torch.float32, device='cuda')
    stats2 = torch.empty(6, dtype=torch.float64, device='cuda')
    P = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(built_lib.mg_ppo_loss(B, P(pred), P(batch.logp), P(batch.adv), P(batch.ret), HP[0], HP[1], HP[2], P(stats2), P(gout),
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.autograd.backward([out['logp'], out['ent'], out['v']], [gout[0], gout[1], gout[2]])
    torch.cuda.synchronize()
    assert torch.equal(ac.theta.grad, want)


@pytest.mark.parametrize('n', [1, 2047, 2049, 185003])
def test_gradient_norm_and_clip_are_repeatable(built_lib, n):
    """accuracy: the tolerances of tests/test_gpu_ppo.py::test_grad_norm_and_clip"""
    import molgym_amd
    from molgym_amd import _lib
    molgym_amd.set_deterministic(True)
    gref = torch.randn(n, generator=torch.Generator().manual_seed(n))
    P = lambda t: C.c_void_p(t.data_ptr())
    for max_norm in (0.5, 1e6):
        first = None
        for _ in range(3):
            gdev = gref.clone().cuda()
            out = torch.zeros(2, device='cuda')
            _lib.check(built_lib.mg_grad_norm_clip(n, P(gdev), max_norm, P(out), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            torch.cuda.synchronize()
            if first is None:
                first = (out[:1].clone(), gdev.clone())
            assert torch.equal(out[:1], first[0]) and torch.equal(gdev, first[1])
        p = torch.nn.Parameter(torch.zeros_like(gref))
        p.grad = gref.clone()
        norm = torch.nn.utils.clip_grad_norm_([p], max_norm)
        assert abs(first[0].item() - norm.item()) / norm.item() < 1e-5
        assert torch.allclose(first[1].cpu(), p.grad, rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize('target_kl,steps', [(1e9, 3), (0.01, 0)], ids=['runs_all_epochs', 'stops_early'])
def test_train_twice_gives_the_same_bits(built_lib, monkeypatch, target_kl, steps):
    """70 samples in mini-batches of 20 (three full ones and a ragged one of 10), three epochs, twice from copies of one agent.
    The recorded log-probs sit 0.05 above the agent's own, so the first epoch's approx_kl is 0.05: far below 1.5e9, above 0.015."""
    import molgym_amd
    from molgym_amd import ppo
    molgym_amd.set_deterministic(True)
    base = _agent(12, 64, 7)
    data = make_batch_internal(70, 7, ZS, seed=21)
    with torch.no_grad():
        data['logp'] = base.step(data['obs'], data['act'])['logp'].double().cpu().numpy() + 0.05
    runners = []

    class Recording(ppo._DeviceRunner):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            runners.append(self)

    monkeypatch.setattr(ppo, '_DeviceRunner', Recording)
    runs = []
    for _ in range(2):
        ac = copy.deepcopy(base)
        opt = torch.optim.Adam(ac.parameters(), lr=3e-4)
        np.random.seed(5)
        infos = ppo.train(ac, opt, data, mini_batch_size=20, clip_ratio=0.2, target_kl=target_kl, vf_coef=0.5, entropy_coef=0.01,
                          gradient_clip=0.5, max_num_steps=3)
        torch.cuda.synchronize()
        st = opt.state.get(ac.theta, {})
        runs.append((infos, ac.theta.detach().clone(), st.get('exp_avg'), st.get('exp_avg_sq')))
    assert len(runners) == 2 and all(len(r.streams) <= 1 for r in runners)
    a, b = runs
    assert a[0]['num_opt_steps'] == b[0]['num_opt_steps'] == steps
    assert set(a[0]) == set(b[0])
    for k in a[0]:
        if k != 'time':
            assert a[0][k] == b[0][k], (k, a[0][k], b[0][k])
    assert torch.equal(a[1], b[1])
    assert (steps > 0) == (not torch.equal(a[1], base.theta.detach()))
    for x, y in zip(a[2:], b[2:]):
        assert (x is None and y is None) or torch.equal(x, y)
    if steps:
        assert a[2] is not None and a[3] is not None


def test_covariant_agent_refuses(built_lib):
    import molgym_amd
    from molgym_amd.synthetic import make_batch
    from tests.helpers import make_pair
    ac, _, cfg = make_pair('cfg2', seed=3)
    data = make_batch(6, cfg['canvas_size'], cfg['zs'], seed=2)
    batch = ac.prepare_batch(data['obs'], data['act'], data['logp'], data['adv'], data['ret'])
    out = ac.step(data['obs'], data['act'])
    molgym_amd.set_deterministic(True)
    with pytest.raises(RuntimeError, match='deterministic mode covers SchNetAC only'):
        ac.ppo_minibatch(batch, *HP)
    with pytest.raises(RuntimeError, match='deterministic mode covers SchNetAC only'):
        out['logp'].sum().backward()
    molgym_amd.set_deterministic(False)
    ac.ppo_minibatch(batch, *HP)  # and nothing sticks
    torch.cuda.synchronize()
    assert torch.isfinite(ac.theta.grad).all()
