"""SchNetAC.step_canvas: the internal-coordinate agent's rollout step on device-resident canvases (mg_int_sample_ids).
The z-matrix placement against the host's float64 helper, evaluation mode against step(obs), the drawn rows against their
own evaluation and their distributions, keyed streams, canvas tracking and rollouts."""
import ctypes as C

import numpy as np
import pytest
import torch

from molgym_amd import _lib, ppo
from molgym_amd.buffer import PPOBufferContainer
from molgym_amd.env_container import SimpleEnvContainer
from molgym_amd.spaces import ActionSpace, ObservationSpace
from molgym_amd.synthetic import make_batch
from tests.fake_env import FakeMolEnv
from tests.helpers import make_pair, rel_err

pytestmark = pytest.mark.gpu
ZS = [0, 9, 16]


def _agent(seed, canvas=7, width=64):
    from molgym_amd.agents.internal import SchNetAC
    torch.manual_seed(seed)
    ac = SchNetAC(ObservationSpace(canvas, ZS), ActionSpace(ZS), (0.8, 1.8), width, device='cuda:0')
    with torch.no_grad():  # non-zero biases: every head depends on its inputs
        g = torch.Generator().manual_seed(seed + 1)
        for name, (off, shape) in ac.slot_table.items():
            n = int(np.prod(shape))
            if name.endswith('bias'):
                ac.theta[off:off + n] = (0.1 * torch.randn(n, generator=g)).to(ac.theta)
    return ac


def _place_dev(pos64, natoms, acts):
    dev = torch.device('cuda:0')
    B, N, _ = pos64.shape
    p = torch.from_numpy(np.ascontiguousarray(pos64)).to(dev)
    n = torch.from_numpy(np.asarray(natoms, dtype=np.int32)).to(dev)
    a = torch.from_numpy(np.ascontiguousarray(acts, dtype=np.float32)).to(dev)
    plus = torch.empty(B, 3, dtype=torch.float64, device=dev)
    minus = torch.empty_like(plus)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().mg_int_place(B, N, ptr(p), ptr(n), ptr(a), ptr(plus), ptr(minus),
                                           C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return plus.cpu().numpy(), minus.cpu().numpy()


def _place_host(pos64, natoms, acts):
    from molgym_amd.agents.internal import place_new_atoms
    a64 = np.asarray(acts, dtype=np.float32).astype(np.float64)
    focus = np.rint(a64[:, 1]).astype(np.int64)
    return (place_new_atoms(pos64, natoms, focus, a64[:, 3], a64[:, 4], a64[:, 5]),
            place_new_atoms(pos64, natoms, focus, a64[:, 3], a64[:, 4], -a64[:, 5]))


def _sf6(order):
    """an exact SF6 octahedron (S at the origin, F on the axes at 1.56) in the given slot order of the six F"""
    axes = [(1, 0, 0), (0, 1, 0), (-1, 0, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    return np.array([(0.0, 0.0, 0.0)] + [tuple(1.56 * c for c in axes[i]) for i in order], dtype=np.float64)


def test_placement_matches_the_host_helper(built_lib):
    N = 9
    rng = np.random.default_rng(5)
    cases = []
    for n in (0, 1, 2, 3, N):
        for _ in range(6):
            cases.append((rng.normal(scale=1.5, size=(N, 3)), n))
    sf6 = np.zeros((N, 3))
    sf6[:7] = _sf6([0, 1, 2, 3, 4, 5])
    for f in range(7):  # every focus of the octahedron: ties among the nearest atoms everywhere
        cases.append((sf6, 7, f))
    B = len(cases)
    pos = np.zeros((B, N, 3))
    natoms = np.zeros(B, dtype=np.int32)
    acts = np.zeros((B, 7), dtype=np.float32)
    for b, c in enumerate(cases):
        pos[b], natoms[b] = c[0], c[1]
        pos[b, natoms[b]:] = 0.0
        acts[b, 1] = c[2] if len(c) > 2 else rng.integers(0, max(c[1], 1))
        acts[b, 3:6] = (rng.uniform(0.8, 1.8), rng.uniform(0.3, 2.8), rng.uniform(-3.0, 3.0))
    got_p, got_m = _place_dev(pos, natoms, acts)
    want_p, want_m = _place_host(pos, natoms, acts)
    assert np.all(np.isfinite(got_p)) and np.all(np.isfinite(got_m))
    assert np.abs(got_p - want_p).max() <= 1e-12 and np.abs(got_m - want_m).max() <= 1e-12
    # the tie order decides: focus on the first F (slot 1); its four cis neighbours are equally far, and the z-matrix reference
    # is the FIRST of them in slot order.  Another slot order of the same molecule moves the atom by far more than 1e-3, and
    # the device follows the slot order exactly as the host does.
    pos2 = np.zeros((2, N, 3))
    pos2[0, :7], pos2[1, :7] = _sf6([0, 1, 2, 3, 4, 5]), _sf6([0, 4, 2, 3, 1, 5])
    a2 = np.array([[0, 1, 0, 1.2, 1.9, 2.2, 0]] * 2, dtype=np.float32)
    want = _place_host(pos2, np.array([7, 7]), a2)[0]
    got = _place_dev(pos2, np.array([7, 7]), a2)[0]
    assert np.abs(want[0] - want[1]).max() > 1e-3
    assert np.abs(got - want).max() <= 1e-12


@pytest.mark.parametrize('canvas', [7, 20])
def test_evaluation_mode_matches_step_obs(built_lib, canvas):
    """training = False: argmax / means on both paths, so the rows agree (N + 1 > 16 at canvas 20: the grouped head kernels)"""
    ac = _agent(3, canvas=canvas, width=128 if canvas == 7 else 64)
    ac.training = False
    obs = make_batch(140, canvas, ZS, seed=4)['obs']
    cv = ac.make_canvas(obs)
    with torch.no_grad():
        got = ac.step_canvas(cv, commit=False)
        kv = ac._ws_view(ac._last_sample_cfg, ac._last_ws, 'kv')[:2 * len(obs)].view(2, -1).t().cpu().numpy()
        want = ac.step(obs)
    assert cv.matches(obs)
    ga, wa = got['a'].cpu().numpy(), want['a'].cpu().numpy()
    assert np.array_equal(ga[:, :3], wa[:, :3])
    assert np.abs(ga[:, 3:6] - wa[:, 3:6]).max() <= 1e-6
    close = np.abs(kv[:, 0] - kv[:, 1]) < 1e-5
    same = ga[:, 6] == wa[:, 6]
    assert np.all(same | close)
    rows = np.nonzero(same)[0]
    assert len(rows) > 100
    for k in ('logp', 'ent', 'v'):
        assert rel_err(got[k][rows], want[k][rows]) < 1e-5, k
    for b in rows:
        (e1, p1), (e2, p2) = got['actions'][b], want['actions'][b]
        assert e1 == e2
        assert np.abs(np.subtract(p1, p2)).max() <= 1e-9


def test_training_draws_are_consistent_with_their_evaluation(built_lib):
    ac = _agent(6)
    ac.training = True
    data = make_batch(64, 7, ZS, seed=8)
    cv = ac.make_canvas(data['obs'])
    with torch.no_grad():
        got = ac.step_canvas(cv, commit=False, seed=1234)
        a = got['a'].cpu().numpy()
        again = ac.step(data['obs'], a)
    for k in ('logp', 'ent', 'v'):
        assert rel_err(got[k], again[k]) < 1e-5, k
    for (e1, p1), (e2, p2) in zip(got['actions'], again['actions']):
        assert e1 == e2 and np.abs(np.subtract(p1, p2)).max() <= 1e-9
    natoms = cv.natoms
    assert np.all(a[:, 0] == 0) and np.all(a[:, 1] < np.maximum(natoms, 1)) and np.all(a[:, 3] >= 0.001)
    for b, (_, bag) in enumerate(data['obs']):
        assert bag[int(a[b, 2])] > 0 or not any(c > 0 for c in bag)
    assert set(np.unique(a[:, 6])) <= {0.0, 1.0}


@pytest.mark.parametrize('which', ['full', 'one', 'empty'])
def test_draw_frequencies_follow_the_distributions(built_lib, which):
    ac = _agent(9)
    ac.training = True
    data = make_batch(16, 7, ZS, seed=3)
    count = lambda o: sum(1 for it in o[0] if ZS[it[0]] != 0)
    full = max(data['obs'], key=count)
    keep = {'full': 7, 'one': 1, 'empty': 0}[which]
    ob = (tuple(full[0][:keep]) + ((0, (0.0, 0.0, 0.0)), ) * (7 - keep), full[1])
    ob = (ob[0], (0, 2, 1))  # two elements in the bag
    E = 512
    obs = [ob] * E
    cv = ac.make_canvas(obs)
    with torch.no_grad():
        got = ac.step_canvas(cv, commit=False, seed=77)
    a = got['a'].cpu().numpy()
    cfg, ws = ac._last_sample_cfg, ac._last_ws
    n = count(ob)
    view = lambda name, cnt: ac._ws_view(cfg, ws, name)[:cnt].double().cpu().numpy()
    sig = lambda p: 4.0 * np.sqrt(np.maximum(p * (1 - p), 1e-4) / E)
    if n > 0:  # focus
        p = torch.softmax(torch.from_numpy(view('logitF', n)), 0).numpy()
        freq = np.bincount(a[:, 1].astype(int), minlength=n)[:n] / E
        assert np.all(np.abs(freq - p) <= sig(p))
    else:
        assert np.all(a[:, 1] == 0)
    # element (every row has the same focus distribution, not the same focus: check the mixture over the drawn foci by
    # re-reading the per-row logits of the final pass)
    le = view('logitE', E * 3).reshape(E, 3)
    mask = np.array(ob[1]) > 0
    pe = np.where(mask, np.exp(le - le.max(1, keepdims=True)), 0.0)
    pe = (pe / pe.sum(1, keepdims=True)).mean(0)
    freq = np.bincount(a[:, 2].astype(int), minlength=3) / E
    assert np.all(np.abs(freq - pe) <= sig(pe))
    # continuous: standardised residuals of the draws
    co = view('cout', E * 3).reshape(E, 3)
    o, _ = ac.slot_table['log_stds']
    sd = np.exp(1e-6 + ac.theta[o:o + 3].detach().double().cpu().numpy())
    half = np.array([0.5, 0.5 * np.pi, 0.5 * np.pi])
    cen = np.array([1.3, 0.5 * np.pi, 0.5 * np.pi])
    mean = np.tanh(co) * half + cen
    zres = (a[:, 3:6] - mean) / sd
    keep = np.ones(E, dtype=bool) if mean[:, 0].min() - 4 * sd[0] > 0.001 else a[:, 3] > 0.001  # (the clamp)
    for k in range(3):
        zk = zres[keep, k]
        assert abs(zk.mean()) <= 4.0 / np.sqrt(len(zk)), k
        assert abs(zk.std() - 1.0) <= 4.0 * np.sqrt(0.5 / len(zk)), k
    assert a[:, 3].min() >= 0.001
    # kappa
    kv = view('kv', 2 * E).reshape(2, E).T
    pk = np.exp(kv[:, 1]) / (np.exp(kv[:, 0]) + np.exp(kv[:, 1]))
    assert abs(a[:, 6].mean() - pk.mean()) <= 4.0 * np.sqrt(max(pk.mean() * (1 - pk.mean()), 1e-4) / E)


def test_keyed_streams_reproduce_rows_across_groups(built_lib):
    ac = _agent(12)
    ac.training = True
    obs = make_batch(24, 7, ZS, seed=6)['obs']
    with torch.no_grad():
        full = ac.step_canvas(ac.make_canvas(obs), commit=False, seed=99)
        halves = [ac.step_canvas(ac.make_canvas(obs[g::2]), commit=False, seed=99, sample_ids=(g, 2)) for g in range(2)]
        other = ac.step_canvas(ac.make_canvas(obs), commit=False, seed=100)
    fa = full['a'].cpu().numpy()
    for g in range(2):
        assert np.array_equal(halves[g]['a'].cpu().numpy(), fa[g::2])
        for k in ('logp', 'ent', 'v'):
            assert torch.equal(halves[g][k].cpu(), full[k].cpu()[g::2]), k
        assert halves[g]['actions'] == full['actions'][g::2]
    assert not np.array_equal(other['a'].cpu().numpy(), fa)


def test_canvas_tracks_the_environments(built_lib):
    ac = _agent(21)
    ac.training = True
    envs = SimpleEnvContainer([FakeMolEnv(7, ZS, (0, 1 + i % 3, 2 + i % 2)) for i in range(12)])
    obs = envs.reset()
    cv = ac.make_canvas(obs)
    assert cv.matches(obs)
    resets = 0
    for it in range(9):
        with torch.no_grad():
            got = ac.step_canvas(cv, seed=500 + it)
        next_obs, _, terminals, _ = envs.step(got['actions'])
        alive = np.nonzero(~np.asarray(terminals))[0]
        if len(alive):
            assert cv.matches([next_obs[i] for i in alive], alive)
        obs = envs.reset_if_terminal(next_obs, terminals)
        resets += int(np.sum(terminals))
        stale = cv.stale_rows(obs, terminals)
        assert set(np.nonzero(terminals)[0]) <= set(stale)
        cv.sync(stale, [obs[i] for i in stale])
        assert cv.matches(obs)
    assert resets > 0
    with torch.no_grad():
        ac.step_canvas(cv, commit=False)
    assert cv.matches(obs)


def test_rollouts_on_canvas_serial_equals_pipelined_and_stay_opt_in(built_lib):
    from molgym_amd.env_container import AsyncEnvContainer
    ac = _agent(31)
    assert not ppo._use_canvas(ac)  # the default: SchNetAC rollouts keep step(obs) and torch's RNG
    cov, _, _ = make_pair('cfg2', seed=3)
    assert ppo._use_canvas(cov)
    ac.rollout_on_canvas = True
    assert ppo._use_canvas(ac)
    calls = []
    orig = ac.step

    def no_step(observations, actions=None):  # the rollout must not fall back to the parsing path
        calls.append(actions is None)
        return orig(observations, actions)

    ac.step = no_step
    mk = lambda: [FakeMolEnv(7, ZS, (0, 1 + i % 3, 2 + i % 2)) for i in range(8)]
    results = {}
    for kind in ('serial', 'pipelined'):
        envs = SimpleEnvContainer(mk()) if kind == 'serial' else AsyncEnvContainer(mk(), num_workers=2, start_method='forkserver')
        try:
            cont = PPOBufferContainer(size=8, gamma=0.99, lam=0.97)
            torch.manual_seed(11)
            ppo.batch_rollout(ac, envs, cont, num_steps=8 * 6, pipeline=2)  # (SimpleEnvContainer: the serial loop)
            results[kind] = cont.merge()
        finally:
            if kind == 'pipelined':
                envs.close()
    assert not any(calls)
    a, b = results['serial'], results['pipelined']
    assert a.obs_buf == b.obs_buf and a.term_buf == b.term_buf
    for f in ('act_buf', 'rew_buf', 'val_buf', 'logp_buf', 'adv_buf', 'ret_buf'):
        assert np.array_equal(np.asarray(getattr(a, f), dtype=np.float64), np.asarray(getattr(b, f), dtype=np.float64)), f
