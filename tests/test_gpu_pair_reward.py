"""`mg_traj_pair_reward` and `DeviceRollout(reward=PairReward(...))` against the float64 host mirror `PairReward.host`: the kernel
alone on hand-filled stores (bit equality, guard bands, untouched slots), the device path of `collect` against the existing
host path with the same reward (`reward_fn=R.host`, which the existing suite holds to the host loop), a reward whose host
mirror raises, refills with a start structure against their host loop, and a shard.

Float64 `/` and `sqrt` are correctly rounded on the device and contraction is off, so every comparison is exact.

The reward of the path tests: eps = (0, 0.08, 0.10, 0.12), sigma = (0, 1.35, 1.45, 1.40) for zs = (0, 1, 6, 8), no cutoff, no
penalty; min_reward -0.25 at a minimum atomic distance of 1.2.  Histograms of the host-path runs (24 steps, 6 environments):
  CovariantAC seed 0: PLACED 86, TOO_CLOSE 17, SOLO 19, BAG_EMPTY 6, LOW_REWARD 16; the paid PLACED rewards lie in -0.2226 .. 0.1633
  SchNetAC seed 5:    PLACED 96, TOO_CLOSE 10, SOLO 24, BAG_EMPTY 9, LOW_REWARD 5;  the paid PLACED rewards lie in -0.2221 .. 0.1052
  shard (1, 2) of 5:  PLACED 43, TOO_CLOSE 8, SOLO 10, BAG_EMPTY 2, LOW_REWARD 9
  refills, water start, canvas 8, minimum distance 1.0: PLACED 41, TOO_CLOSE 34, SOLO 13, LOW_REWARD 56 -- 55 cuts of a PLACED step
  and one of a REFILLED step (the only refill of the run, so no REFILLED is left in the histogram)"""
import ctypes as C

import numpy as np
import pytest
import torch

from molgym_amd import _lib
from molgym_amd.rewards import PairReward
from molgym_amd.rollout import DeviceRollout
from tests import episode_rules_ref as X
from tests import traj_ref as J
from tests.test_gpu_device_rollout import (BAGS, FORMULAS, GAMMA, LAM, MAX_SOLO, MIN_D, MIN_REWARD, SEED, STEPS, WATER, ZS, _agent,
                                           _histogram, host_rollout)

pytestmark = pytest.mark.gpu
GUARD = 4096
ATOM = (J.PLACED, J.FULL, J.BAG_EMPTY, X.REFILLED)

# ---- 1. the kernel alone ---------------------------------------------------------------------------------------------------------
K_ZS = [1, 6, 8]
# all six eps_ij and all six sigma_ij differ: a transposed or mis-indexed lookup changes the reward
K_EPS = np.array([[0.050, 0.071, 0.093], [0.071, 0.110, 0.127], [0.093, 0.127, 0.160]])
K_SIGMA = np.array([[1.10, 1.27, 1.21], [1.27, 1.52, 1.46], [1.21, 1.46, 1.38]])
K_PENALTY, K_CUTOFF = 0.015, 3.1
E, T, STEP = 5, 3, 1
# per launch: five rows of (status, alive, atoms before the step, coincident with an atom of the row?).  min_reward IS the middle
# one of the finite rewards the launch pays (with three or more of them, rewards lie on both sides of it).  N = 70: the counts 0, 1, 63, 64, 65, 69 -- the lane stride wraps and the fold crosses the 64-lane seam
LAUNCHES = {
    '7a': (7, [(J.PLACED, 1, 0, False), (X.REFILLED, 1, 1, False), (J.FULL, 1, 6, False), (J.STOP, 1, 3, False), (J.INACTIVE, 1, 5, False)]),
    '7b': (7, [(J.BAG_EMPTY, 1, 3, False), (J.PLACED, 1, 4, True), (J.PLACED, 0, 5, False), (J.TOO_CLOSE, 1, 4, False), (J.PLACED, 1, 5, False)]),
    '70a': (70, [(J.PLACED, 1, 0, False), (X.REFILLED, 1, 1, False), (J.FULL, 1, 69, False), (J.STOP, 1, 63, False), (J.INACTIVE, 1, 5, False)]),
    '70b': (70, [(J.BAG_EMPTY, 1, 63, False), (J.PLACED, 1, 64, False), (J.PLACED, 0, 65, False), (J.TOO_CLOSE, 1, 64, False),
                 (J.PLACED, 1, 65, True)]),
    '70c': (70, [(X.REFILLED, 1, 65, False), (J.PLACED, 1, 69, False), (J.BAG_EMPTY, 1, 64, False), (J.SOLO, 1, 69, False),
                 (J.FULL, 1, 69, True)]),
    '255': (255, [(J.FULL, 1, 254, False), (J.PLACED, 1, 254, True), (J.PLACED, 1, 200, False), (J.BAG_EMPTY, 1, 128, False),
                  (J.PLACED, 0, 254, False)]),
}


def kernel_reward():
    return PairReward(K_ZS, K_EPS, K_SIGMA, distance_penalty=K_PENALTY, cutoff=K_CUTOFF)


def kernel_case(name):
    """the inputs of one launch and what it must leave behind, all on the host (no device needed): dict of arrays"""
    N, rows = LAUNCHES[name]
    R = kernel_reward()
    rng = np.random.RandomState(sum(ord(c) for c in name))
    # a molecule: the n sites of a jittered 7 x 7 x 6 lattice of spacing 1.45 (no two atoms closer than 1.0) nearest to one of
    # them; the new atom goes to the next nearest, on the surface of the cluster
    sites = np.array([(i, j, k) for i in range(7) for j in range(7) for k in range(6)], dtype=np.float64) * 1.45 - np.array([4.35, 4.35, 3.6])
    S = E * T
    pos = np.full((S, N, 3), np.nan)  # slots beyond the count are never read: NaN would surface as -inf
    charges = np.full((S, N), 99, dtype=np.int32)  # (and 99 is no element of zs)
    newpos, element = rng.normal(size=(E, 3)), rng.randint(0, 3, size=E).astype(np.int32)
    natoms = np.array([r[2] for r in rows], dtype=np.int32)
    status, alive = np.array([r[0] for r in rows], dtype=np.int32), np.array([r[1] for r in rows], dtype=np.int32)
    for s in range(S):  # every slot holds a molecule, so a read of the wrong slot gives a wrong number, not a NaN
        e = s // T
        order = np.argsort(np.linalg.norm(sites - sites[rng.randint(len(sites))], axis=1) + rng.uniform(0.0, 0.1, size=len(sites)))
        n = int(natoms[e])
        pos[s, :n] = sites[order[:n]] + rng.uniform(-0.2, 0.2, size=(n, 3))
        charges[s, :n] = rng.choice(K_ZS, size=n)
        if s % T == STEP:
            newpos[e] = sites[order[n]] + rng.uniform(-0.2, 0.2, size=3)
            if rows[e][3]:
                newpos[e] = pos[s, n // 2]
    rew0 = 1000.0 + np.arange(S, dtype=np.float64)  # the sentinel of s_rew: what mg_traj_status or an earlier step left there
    paying = [e for e in range(E) if status[e] in ATOM and alive[e]]
    before = [(charges[e * T + STEP, :natoms[e]], pos[e * T + STEP, :natoms[e]]) for e in paying]
    r = R.host(before, np.array([K_ZS[element[e]] for e in paying]), newpos[paying], np.array(paying))
    finite = np.sort(r[np.isfinite(r)])
    min_reward = float(finite[len(finite) // 2])
    pivot = paying[int(np.nonzero(r == min_reward)[0][0])]
    want_rew, want_out, want_flags = rew0.copy(), np.zeros(E), np.zeros(E, dtype=np.int32)
    for k, e in enumerate(paying):
        want_rew[e * T + STEP], want_out[e], want_flags[e] = r[k], r[k], 0 if r[k] >= min_reward else 1
    # how many pairs the cutoff drops and keeps
    dropped = kept = 0
    for k, e in enumerate(paying):
        d = before[k][1] - newpos[e]
        r2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        dropped, kept = dropped + int((r2 > R.cutoff2).sum()), kept + int((r2 <= R.cutoff2).sum())
    return dict(N=N, pos=pos, charges=charges, newpos=newpos, element=element, natoms=natoms, status=status, alive=alive, rew0=rew0,
                min_reward=min_reward, paying=paying, pivot=pivot, r=r, want_rew=want_rew, want_out=want_out, want_flags=want_flags,
                dropped=dropped, kept=kept)


class _Guarded:
    """a device array with the bytes of the host array `init`, between two guard bands of 0xA5"""

    def __init__(self, init):
        host = torch.from_numpy(np.ascontiguousarray(init))
        self.nbytes = host.numel() * host.element_size()
        self.big = torch.full((GUARD + self.nbytes + GUARD, ), 0xA5, dtype=torch.uint8, device='cuda')
        self.t = self.big[GUARD:GUARD + self.nbytes].view(host.dtype)
        self.t.copy_(host)

    def intact(self):
        return bool((self.big[:GUARD] == 0xA5).all()) and bool((self.big[GUARD + self.nbytes:] == 0xA5).all())


def _launch(c, R, out, min_reward=None, **override):
    dev = {k: torch.from_numpy(np.ascontiguousarray(c[k])).cuda() for k in ('pos', 'charges', 'newpos', 'element', 'natoms', 'status', 'alive')}
    four_eps, sigma2 = R.device_tables(torch.device('cuda:0'))
    p = lambda x: C.c_void_p(x.data_ptr())
    a = dict(E=E, T=T, t=STEP, N=c['N'], Z=len(K_ZS), penalty=R.distance_penalty, cutoff2=R.cutoff2,
             min_reward=c['min_reward'] if min_reward is None else min_reward)
    a.update(override)
    rc = _lib.lib().mg_traj_pair_reward(a['E'], a['T'], a['t'], a['N'], a['Z'], (C.c_int32 * len(K_ZS))(*K_ZS), p(four_eps), p(sigma2),
                                        a['penalty'], a['cutoff2'], a['min_reward'], p(dev['status']), p(dev['element']), p(dev['newpos']),
                                        p(dev['natoms']), p(dev['alive']), p(dev['pos']), p(dev['charges']), p(out[0].t), p(out[1].t),
                                        p(out[2].t), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, dev


@pytest.mark.parametrize('name', list(LAUNCHES))
def test_kernel_against_the_host_mirror(built_lib, name):
    c, R = kernel_case(name), kernel_reward()
    # the case is what it claims to be: a coincident atom pays -inf, the pivot row pays exactly min_reward and is not cut, and
    # the launches of a canvas size pay on both sides of it; the cutoff drops some pairs and keeps some
    finite = c['r'][np.isfinite(c['r'])]
    coincident = [e for e in c['paying'] if LAUNCHES[name][1][e][3]]
    assert all(c['want_out'][e] == float('-inf') and c['want_flags'][e] == 1 for e in coincident)
    assert c['want_out'][c['pivot']] == c['min_reward'] and c['want_flags'][c['pivot']] == 0 and np.isfinite(c['min_reward'])
    assert c['kept'] > 0 and (c['dropped'] > 0 or c['N'] == 7), (c['kept'], c['dropped'])
    if len(finite) >= 3:
        assert (finite > c['min_reward']).any() and (finite < c['min_reward']).any(), (finite, c['min_reward'])
    out = (_Guarded(c['rew0']), _Guarded(np.full(E, -777.0)), _Guarded(np.full(E, -7, dtype=np.int32)))
    rc, dev = _launch(c, R, out)
    assert rc == 0, _lib.lib().mg_last_error()
    got_rew, got_out, got_flags = out[0].t.cpu().numpy(), out[1].t.cpu().numpy(), out[2].t.cpu().numpy()
    print(name, 'reward_out', got_out, 'flags', got_flags)
    assert all(o.intact() for o in out)
    assert np.array_equal(got_out, c['want_out']) and np.array_equal(got_flags, c['want_flags'])
    assert np.array_equal(got_rew, c['want_rew'])
    # steps 0 and 2 of every row, and the slot of every row that does not pay, keep the sentinel
    untouched = [s for s in range(E * T) if s % T != STEP or s // T not in c['paying']]
    assert np.array_equal(got_rew[untouched], c['rew0'][untouched]) and len(untouched) == E * T - len(c['paying'])
    # and the inputs are inputs
    for k, t in dev.items():
        assert np.array_equal(t.cpu().numpy(), c[k], equal_nan=True), k


def test_kernel_without_cutoff_and_penalty(built_lib):
    """cutoff2 = +inf keeps every pair; min_reward = +inf flags every paying row, -inf none (a -inf reward included)"""
    c = kernel_case('70b')
    R = PairReward(K_ZS, K_EPS, K_SIGMA)
    before = [(c['charges'][e * T + STEP, :c['natoms'][e]], c['pos'][e * T + STEP, :c['natoms'][e]]) for e in c['paying']]
    r = R.host(before, np.array([K_ZS[c['element'][e]] for e in c['paying']]), c['newpos'][c['paying']], np.array(c['paying']))
    assert not np.array_equal(r, c['r'])
    for min_reward, flag in ((float('inf'), 1), (float('-inf'), 0)):
        out = (_Guarded(c['rew0']), _Guarded(np.full(E, -777.0)), _Guarded(np.full(E, -7, dtype=np.int32)))
        rc, _ = _launch(c, R, out, min_reward=min_reward)
        assert rc == 0 and all(o.intact() for o in out)
        want_out, want_flags = np.zeros(E), np.zeros(E, dtype=np.int32)
        want_out[c['paying']], want_flags[c['paying']] = r, flag
        assert np.array_equal(out[1].t.cpu().numpy(), want_out) and np.array_equal(out[2].t.cpu().numpy(), want_flags)


def test_kernel_refuses_bad_arguments(built_lib):
    c, R = kernel_case('7a'), kernel_reward()
    out = (_Guarded(c['rew0']), _Guarded(np.full(E, -777.0)), _Guarded(np.full(E, -7, dtype=np.int32)))
    bad = [dict(E=0), dict(T=0), dict(t=T), dict(t=-1), dict(N=0), dict(N=256), dict(Z=1), dict(Z=17), dict(min_reward=float('nan')),
           dict(penalty=-0.5), dict(penalty=float('nan')), dict(penalty=float('inf')), dict(cutoff2=0.0), dict(cutoff2=-1.0),
           dict(cutoff2=float('nan')), dict(E=1 << 15, T=1 << 10, N=64)]
    for override in bad:
        assert _launch(c, R, out, **override)[0] == -1, override
    assert b'2^31' in _lib.lib().mg_last_error()
    p = C.c_void_p(out[1].t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    zs = (C.c_int32 * 3)(*K_ZS)
    for k in range(13):  # every pointer argument: zs_host, the two tables, the ten arrays
        ptrs = [None if i == k else p for i in range(13)]
        host_zs = None if k == 0 else zs
        assert _lib.lib().mg_traj_pair_reward(E, T, STEP, 7, 3, host_zs, ptrs[1], ptrs[2], 0.0, 1.0, -0.5, *ptrs[3:], s) == -1, k
    torch.cuda.synchronize()
    assert np.array_equal(out[0].t.cpu().numpy(), c['rew0']) and bool((out[1].t == -777.0).all()) and bool((out[2].t == -7).all())


# ---- 2. the device path of collect against the host path of the same reward -----------------------------------------------------
P_EPS, P_SIGMA = (0.0, 0.08, 0.10, 0.12), (0.0, 1.35, 1.45, 1.40)
PATH_CASES = [('covariant', 0), ('internal', 5)]  # the agent seeds of tests/test_gpu_device_rollout.py at E = 6
E_PATH = 6
_CACHE = {}


def path_reward(cls=PairReward):
    return cls(ZS, P_EPS, P_SIGMA)


def _collect(roll, steps=STEPS):
    """(statistics, the Episodes the steps finished) of one collect"""
    episodes, inner = [], roll.step

    def step(*args, **kw):
        rec = inner(*args, **kw)
        episodes.extend(rec['episodes'])
        return rec

    roll.step = step
    try:
        with torch.no_grad():
            info = roll.collect(steps, seed=SEED)
    finally:
        del roll.step
    return info, episodes


def _paths(kind, agent_seed):
    key = (kind, agent_seed)
    if key not in _CACHE:
        ac, R = _agent(kind, agent_seed), path_reward()
        kw = dict(gamma=GAMMA, lam=LAM, min_reward=MIN_REWARD, min_atomic_distance=MIN_D, max_solo_distance=MAX_SOLO)
        dev, host = DeviceRollout(ac, FORMULAS, E_PATH, STEPS, reward=R, **kw), DeviceRollout(ac, FORMULAS, E_PATH, STEPS, reward_fn=R.host, **kw)
        _CACHE[key] = dict(ac=ac, R=R, kw=kw, dev=dev, host=host, dev_run=_collect(dev), host_run=_collect(host))
    return _CACHE[key]


def _same_info(a, b):
    return all(a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])) for k in set(a) | set(b) if k != 'time')


def _same_episodes(a, b):
    return len(a) == len(b) and all(
        (x.env, x.formula, x.status, x.refills, x.bag) == (y.env, y.formula, y.status, y.refills, y.bag) and np.array_equal(x.numbers, y.numbers)
        and np.array_equal(x.positions, y.positions) and np.array_equal(x.logp, y.logp) and np.array_equal(x.v, y.v) for x, y in zip(a, b))


def _same_mirrors(a, b):
    """the host mirrors two rollouts continue from"""
    ok = np.array_equal(a.canvas.natoms, b.canvas.natoms) and np.array_equal(a.canvas.bags_host, b.canvas.bags_host)
    ok = ok and np.array_equal(a.episode_no, b.episode_no) and np.array_equal(a.formula_no, b.formula_no) and np.array_equal(a.refills, b.refills)
    for x, y in zip(a._open, b._open):
        ok = ok and all(len(p) == len(q) and all(np.array_equal(u, w) for u, w in zip(p, q)) for p, q in zip(x, y))
    return ok


def _same_store(a, b):
    va, vb = a._views(), b._views()
    for name in a._table:
        assert torch.equal(getattr(va, name), getattr(vb, name)), name
    assert len(a._table) == 11


@pytest.mark.parametrize('kind,agent_seed', PATH_CASES)
def test_device_path_equals_the_host_path(built_lib, kind, agent_seed):
    c = _paths(kind, agent_seed)
    dev, host = c['dev'], c['host']
    # from the host-path run alone: a cut, a paid placement, and an atom that ended its episode
    status = host.statuses()
    hist = _histogram(status)
    rew = host._views().rew.cpu().numpy().reshape(E_PATH, STEPS)
    paid = rew[status == J.PLACED]
    print('paid PLACED rewards: min', paid.min() if len(paid) else None, 'max', paid.max() if len(paid) else None)
    assert hist[J.LOW_REWARD] > 0 and hist[J.FULL] + hist[J.BAG_EMPTY] > 0, hist
    assert len(paid) > 0 and (paid != 0.0).any() and (paid >= MIN_REWARD).all()
    assert hist[J.ERROR] == 0 and hist[J.INACTIVE] == 0
    # the device path: the same store, mirrors, statistics and episodes
    _same_store(dev, host)
    assert np.array_equal(dev.statuses(), status)
    assert _same_info(c['dev_run'][0], c['host_run'][0]), (c['dev_run'][0], c['host_run'][0])
    assert len(c['host_run'][1]) > 0 and _same_episodes(c['dev_run'][1], c['host_run'][1])
    assert _same_mirrors(dev, host)
    assert torch.equal(dev.canvas.pos64, host.canvas.pos64) and torch.equal(dev.canvas.natoms_dev, host.canvas.natoms_dev)
    assert torch.equal(dev.canvas.bags, host.canvas.bags) and torch.equal(dev.episode_no_dev, host.episode_no_dev)
    for on_device in (None, True, False):
        a, b = dev.train_data(on_device=on_device), host.train_data(on_device=on_device)
        assert torch.equal(a['adv'], b['adv']) and torch.equal(a['ret'], b['ret']) and torch.equal(a['logp'], b['logp'])
        assert len(a['obs']) == len(b['obs']) == E_PATH * STEPS
    a, b = dev.data(), host.data()
    assert torch.equal(a['adv'], b['adv']) and a['obs'] == b['obs'] and np.array_equal(a['act'], b['act'])


class _NoHost(PairReward):

    def host(self, before, new_z, new_pos, rows):
        raise AssertionError('the device path called the host mirror')

    def reward(self, *args):
        raise AssertionError('the device path called the host mirror')


@pytest.mark.parametrize('kind,agent_seed', PATH_CASES)
def test_device_path_never_calls_the_host_mirror(built_lib, kind, agent_seed):
    c = _paths(kind, agent_seed)
    roll = DeviceRollout(c['ac'], FORMULAS, E_PATH, STEPS, reward=path_reward(_NoHost), **c['kw'])
    info, _ = _collect(roll)
    assert _same_info(info, c['host_run'][0])
    _same_store(roll, c['host'])
    # ... and the host path with it does raise
    with pytest.raises(AssertionError, match='host mirror'):
        _collect(DeviceRollout(c['ac'], FORMULAS, E_PATH, STEPS, reward_fn=path_reward(_NoHost).host, **c['kw']))


# ---- 4. rules and shards ---------------------------------------------------------------------------------------------------------
class PairPayingEnvX(X.RulesEnvX):
    """RulesEnvX paying the pair reward under environment.py:58-70 (as `paying` of tests/test_gpu_device_rollout.py pays its
    stand-in); `cut_from` collects the statuses of the steps that were cut"""
    min_reward, R, cut_from = MIN_REWARD, None, None

    def step(self, action):
        numbers = [self.zs[label] for label, _ in self.atoms]
        positions = np.array([p for _, p in self.atoms], dtype=np.float64).reshape(-1, 3)
        obs, _, done, info = super().step(action)
        s = info['status']
        if s == J.STOP:
            return obs, 0.0, True, info
        if s in (J.TOO_CLOSE, J.SOLO, X.OUTSIDE):
            return obs, self.min_reward, True, info
        reward = self.R.reward(numbers, positions, self.zs[int(action[0])], np.array([float(x) for x in action[1]], dtype=np.float64))
        if reward < self.min_reward:
            reward, done = self.min_reward, True
            self.cut_from.append(s)
            if s in (J.PLACED, X.REFILLED):
                info = {'status': J.LOW_REWARD}
        return obs, reward, done, info


R_EPS, R_SIGMA = P_EPS, P_SIGMA


def test_refills_with_a_start_structure(built_lib):
    """num_refills = 1 on a water start, the setup of tests/test_gpu_device_rollout.py::test_refills_against_their_host_loop:
    the device reward against the host LOOP (Python environments paying the mirror), and a REFILLED step is cut"""
    canvas = 8
    from tests.test_gpu_episodes_env import _agent as agent_of
    ac = agent_of('covariant', 0, ZS, canvas)
    R = PairReward(ZS, R_EPS, R_SIGMA)
    start = tuple(WATER) + ((0, (0.0, 0.0, 0.0)), ) * (canvas - 3)
    PairPayingEnvX.R, PairPayingEnvX.cut_from = R, []
    envs = [PairPayingEnvX(canvas, ZS, BAGS, 1.0, MAX_SOLO, start=WATER, num_refills=1) for _ in range(E_PATH)]
    kw = dict(gamma=GAMMA, lam=LAM, min_reward=MIN_REWARD, max_solo_distance=MAX_SOLO, initial=(start, BAGS[0]), min_atomic_distance=1.0,
              num_refills=1)
    dev, host = DeviceRollout(ac, FORMULAS, E_PATH, STEPS, reward=R, **kw), DeviceRollout(ac, FORMULAS, E_PATH, STEPS, reward_fn=R.host, **kw)
    a, b = _collect(dev), _collect(host)
    # what `_mode_pair` of tests/test_gpu_device_rollout.py asserts (its fourth parameter is named `reward` and goes to
    # `reward_fn`, so the keyword cannot pass through it): statuses, returns and statistics of the host loop
    box, status, stats = host_rollout(ac, envs, STEPS, SEED)
    hist = _histogram(status)
    print('cut from:', PairPayingEnvX.cut_from)
    assert np.array_equal(dev.statuses(), status)
    assert torch.equal(dev._views().ret, box.merge().get_data(device=ac.theta.device)['ret'])
    assert a[0]['return_mean'] == stats['return_mean'] and a[0]['episode_length_mean'] == stats['episode_length_mean']
    assert hist[J.LOW_REWARD] > 0 and X.REFILLED in PairPayingEnvX.cut_from and J.PLACED in PairPayingEnvX.cut_from, (hist, PairPayingEnvX.cut_from)
    # and against the host path, array for array
    _same_store(dev, host)
    assert _same_info(a[0], b[0]) and _same_episodes(a[1], b[1]) and _same_mirrors(dev, host)
    assert torch.equal(dev.refills_dev, host.refills_dev) and torch.equal(dev.formula_no_dev, host.formula_no_dev)


def test_a_shard(built_lib):
    """environments 2 .. 4 of 5 (shard 1 of 2): device reward against host-mirror reward on the same shard"""
    c = _paths('covariant', 0)
    dev = DeviceRollout(c['ac'], FORMULAS, 5, STEPS, reward=c['R'], shard=(1, 2), **c['kw'])
    host = DeviceRollout(c['ac'], FORMULAS, 5, STEPS, reward_fn=c['R'].host, shard=(1, 2), **c['kw'])
    assert dev.E == 3 and dev.lo == 2
    a, b = _collect(dev), _collect(host)
    hist = _histogram(host.statuses())
    assert hist[J.PLACED] > 0 and hist[J.LOW_REWARD] > 0, hist
    _same_store(dev, host)
    assert _same_info(a[0], b[0]) and _same_episodes(a[1], b[1]) and _same_mirrors(dev, host)
    assert np.array_equal(dev.statuses(), host.statuses())
