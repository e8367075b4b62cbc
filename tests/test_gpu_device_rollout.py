"""DeviceRollout (mg_traj_record, mg_traj_status, mg_episode_cut, mg_traj_gae) against the host loop it replaces: the loop of
`ppo._rollout_serial` -- `step_canvas` with the same per-step seeds, Python environments that pay a stand-in reward and apply
environment.py:58-70, `PPOBufferContainer`, `merge().get_data(device)`, `prepare_rollout` -- for both agents.

The stand-in reward is the smallest distance from the new atom to the atoms before it, minus 1.6 (0.0 on an empty canvas), in
float64 numpy; both sides call the same function.  With a minimum atomic distance of 1.2 a placed atom's reward lies above
-0.4, and `MIN_REWARD` = -0.25 cuts the placements closer than 1.35.

Seeds: the agent seeds are those of `CASES` in tests/test_gpu_episodes.py: covariant 0 at E = 6, covariant 1 at E = 70, and for
SchNetAC 5 (its evaluation-mode seed there, here in training mode) in place of 0, whose 24 steps finish no molecule under this
reward.  The histogram of every case is asserted."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from molgym_amd import _lib, ppo, rollout
from molgym_amd.buffer import PPOBufferContainer
from molgym_amd.rollout import DeviceRollout
from tests import episode_ref as R
from tests import episode_rules_ref as X
from tests import traj_ref as J
from tests.helpers import rel_err
from tests.test_gpu_episodes import BAGS, CANVAS, FORMULAS, MAX_SOLO, MIN_D, STEPS, WATER, ZS, _agent

pytestmark = pytest.mark.gpu
GAMMA, LAM, MIN_REWARD, SEED = 0.99, 0.95, -0.25, 11
GUARD = 4096


@pytest.fixture(autouse=True)
def _restore_switches(built_lib):
    prev = (_lib.is_deterministic(), _lib.is_deterministic_covariant())
    yield
    _lib.set_deterministic(prev[0], covariant=prev[1])


def stand_in(positions, q):
    """the reward of an atom at `q` next to atoms at `positions` (n, 3): float64 numpy, nothing else"""
    d = R.distances(positions, q)
    return float(np.min(d) - 1.6) if len(d) else 0.0


def reward_fn(before, new_z, new_pos, rows):
    return np.array([stand_in(b[1], q) for b, q in zip(before, new_pos)], dtype=np.float64)


def paying(base):
    """`base` (RulesEnv / RulesEnvX) paying `stand_in` under environment.py:58-70"""

    class Paying(base):
        min_reward, pays = MIN_REWARD, True

        def step(self, action):
            before = np.array([p for _, p in self.atoms], dtype=np.float64).reshape(-1, 3)
            obs, _, done, info = super().step(action)
            s = info['status']
            if s == R.STOP:
                return obs, 0.0, True, info
            if s in (R.TOO_CLOSE, R.SOLO, X.OUTSIDE):
                return obs, self.min_reward, True, info  # an invalid action
            reward = stand_in(before, np.array([float(x) for x in action[1]], dtype=np.float64)) if self.pays else 0.0
            if reward < self.min_reward:
                reward, done = self.min_reward, True
                if s in (R.PLACED, X.REFILLED):
                    info = {'status': J.LOW_REWARD}
            return obs, reward, done, info

    return Paying


PayingEnv, PayingEnvX = paying(R.RulesEnv), paying(X.RulesEnvX)


def _seeds(seed, T):
    gen = torch.Generator().manual_seed(seed)
    return [int(torch.randint(0, 2**62, (1, ), generator=gen).item()) for _ in range(T + 1)]


def host_rollout(ac, envs, T, seed):
    """the loop of ppo._rollout_serial with explicit seeds; returns (container, statuses (E, T), batch_rollout's statistics)"""
    E = len(envs)
    box = PPOBufferContainer(size=E, gamma=GAMMA, lam=LAM)
    seeds = _seeds(seed, T)
    obs = [env._obs() for env in envs]
    cv = ac.make_canvas(obs)
    status = np.zeros((E, T), dtype=np.int32)
    with torch.no_grad():
        for t in range(T):
            pred = ac.step_canvas(cv, seed=seeds[t])
            nxt, rewards, terminals = [], [], []
            for e, env in enumerate(envs):
                env.draw_key = (seeds[t], e)
                o, r, done, info = env.step(pred['actions'][e])
                nxt.append(o)
                rewards.append(r)
                terminals.append(done)
                status[e, t] = info['status']
            a, v, logp = ppo._host_predictions(pred)
            box.store(observations=obs, actions=a, rewards=np.array(rewards, dtype=np.float64), next_observations=nxt,
                      terminals=np.array(terminals), values=v, logps=logp)
            obs = [env.reset() if done else o for env, o, done in zip(envs, nxt, terminals)]
            stale = cv.stale_rows(obs, terminals)
            cv.sync(stale, [obs[i] for i in stale])
        last = ac.step_canvas(cv, commit=False, seed=seeds[T])
        box.finish_paths(ppo._host_predictions(last)[1])
    stats = dict(return_mean=np.mean(box.episodic_returns).item(), return_std=np.std(box.episodic_returns).item(),
                 episode_length_mean=np.mean(box.episode_lengths).item(), episode_length_std=np.std(box.episode_lengths).item())
    return box, status, stats


_CACHE = {}


def _pair(kind, agent_seed, E):
    """one device collect and one host loop per case, shared by the tests that read them (neither is changed afterwards)"""
    key = (kind, agent_seed, E)
    if key not in _CACHE:
        ac = _agent(kind, agent_seed)
        roll = DeviceRollout(ac, FORMULAS, E, STEPS, gamma=GAMMA, lam=LAM, min_reward=MIN_REWARD, reward_fn=reward_fn,
                             min_atomic_distance=MIN_D, max_solo_distance=MAX_SOLO)
        with torch.no_grad():
            info = roll.collect(STEPS, seed=SEED)
        envs = [PayingEnv(CANVAS, ZS, BAGS, MIN_D, MAX_SOLO) for _ in range(E)]
        box, status, stats = host_rollout(ac, envs, STEPS, SEED)
        merged = box.merge()
        _CACHE[key] = dict(ac=ac, roll=roll, info=info, box=box, merged=merged, status=status, stats=stats,
                           data=merged.get_data(device=ac.theta.device))
    return _CACHE[key]


def _histogram(status):
    hist = np.bincount(status.reshape(-1), minlength=11)
    print('statuses:', {rollout.STATUS_NAMES[i]: int(n) for i, n in enumerate(hist) if n})
    return hist


CASES = [('covariant', 0, 6), ('covariant', 1, 70), ('internal', 5, 6)]


@pytest.mark.parametrize('kind,agent_seed,E', CASES)
def test_collect_equals_the_host_loop(built_lib, kind, agent_seed, E):
    c = _pair(kind, agent_seed, E)
    roll, status, data = c['roll'], c['status'], c['data']
    hist = _histogram(status)
    # not vacuous: a placement, a finished molecule, a rule rejection, a cut, and a row still open at the end
    assert hist[J.PLACED] > 0 and hist[J.BAG_EMPTY] + hist[J.FULL] > 0 and hist[J.TOO_CLOSE] + hist[J.SOLO] > 0, hist
    assert hist[J.LOW_REWARD] > 0 and int((~np.isin(status[:, -1], J.ENDS)).sum()) > 0, hist
    assert hist[J.ERROR] == 0 and hist[J.INACTIVE] == 0
    assert np.array_equal(roll.statuses(), status)
    for k in ('return_mean', 'return_std', 'episode_length_mean', 'episode_length_std'):
        assert c['info'][k] == c['stats'][k], (k, c['info'][k], c['stats'][k])
    got = roll.train_data()
    assert len(got['obs']) == E * STEPS and set(got) == set(data)
    for k in ('logp', 'adv', 'ret'):
        assert got[k].dtype == torch.float64 and torch.equal(got[k], data[k]), k
    if kind == 'covariant':
        want = c['ac'].prepare_rollout(data)
        mine = c['ac'].prepare_rollout(got)
        assert mine is got['obs'].rollout and np.array_equal(mine.natoms, want.natoms)
        for name, a, b in zip(('pos', 'charges', 'bags', 'actions', 'logp', 'adv', 'ret'), mine.t, want.t):
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), name
    else:
        host = roll.data()
        assert len(host['obs']) == len(c['merged'].obs_buf)
        for s, (a, b) in enumerate(zip(host['obs'], c['merged'].obs_buf)):
            assert a == b, s
        assert np.array_equal(host['act'], np.array(c['merged'].act_buf)) and host['act'].dtype == np.float32
        assert np.array_equal(got['act'], host['act'])


@pytest.mark.parametrize('kind,agent_seed,E', CASES)
def test_gae_against_the_host_float64_buffers(built_lib, kind, agent_seed, E):
    """adv / ret of the store against `get_data()` on the host, at the tolerance tests/test_gpu_ppo.py holds mg_gae to against
    golden vector G2 (rtol 1e-12, atol 1e-14; the standardised advantages rtol 1e-11, atol 1e-13)"""
    c = _pair(kind, agent_seed, E)
    v, merged = c['roll']._views(), c['merged']
    # the standardised advantages are all the store keeps of adv: re-run the recursion on the host from the store's own inputs
    status = c['roll'].statuses()
    adv, ret, num_done, _, _ = J.segmented_gae(status, v.rew.cpu().numpy(), v.val.cpu().numpy(), c['roll']._last_val.cpu().numpy(), GAMMA, LAM)
    assert np.array_equal(adv.reshape(-1), np.array(merged.adv_buf)) and np.array_equal(ret.reshape(-1), np.array(merged.ret_buf))
    assert np.array_equal(v.rew.cpu().numpy(), np.array(merged.rew_buf)) and int(num_done.sum()) == len(c['box'].episode_lengths)
    host = merged.get_data()
    np.testing.assert_allclose(v.ret.cpu().numpy(), host['ret'], rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(v.adv.cpu().numpy(), host['adv'], rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(v.logp.cpu().numpy(), host['logp'], rtol=0, atol=0)


def _same_info(a, b):
    """the statistics of two collects are equal (NaN, no finished episode, equals NaN)"""
    return all(a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])) for k in set(a) | set(b) if k != 'time')


@pytest.mark.parametrize('byte', [0xFF, 0x7F])
def test_poisoned_store_between_guard_bands(built_lib, byte):
    """every slot of a collect of exactly `capacity` steps is written, nothing outside the reported size is"""
    E, kind, agent_seed = 6, 'covariant', 0
    c = _pair(kind, agent_seed, E)
    ac = c['ac']
    nbytes = rollout.store_layout(E, STEPS, CANVAS, len(ZS), 6)[1]
    big = torch.full((GUARD + nbytes + GUARD, ), 0xA5, dtype=torch.uint8, device='cuda')
    big[GUARD:GUARD + nbytes].fill_(byte)
    roll = DeviceRollout(ac, FORMULAS, E, STEPS, gamma=GAMMA, lam=LAM, min_reward=MIN_REWARD, reward_fn=reward_fn,
                         store=big[GUARD:GUARD + nbytes], min_atomic_distance=MIN_D, max_solo_distance=MAX_SOLO)
    assert roll.store_bytes == nbytes and roll.store.data_ptr() == big.data_ptr() + GUARD
    with torch.no_grad():
        roll.collect(STEPS, seed=SEED)
    torch.cuda.synchronize()
    assert bool((big[:GUARD] == 0xA5).all()) and bool((big[GUARD + nbytes:] == 0xA5).all())
    v, w = roll._views(), c['roll']._views()
    word4, word8 = int.from_bytes(bytes([byte] * 4), 'little', signed=True), int.from_bytes(bytes([byte] * 8), 'little', signed=True)
    for name, (off, dtype, k) in roll._table.items():
        a = getattr(v, name)
        raw = a.view(torch.int64) if dtype == torch.float64 else a.view(torch.int32)
        assert a.numel() == E * STEPS * k and not bool((raw == (word8 if dtype == torch.float64 else word4)).any()), name
        assert torch.equal(a, getattr(w, name)), name  # and the collect is the one of the clean store


def test_second_collect_and_shorter_collect(built_lib):
    E = 6
    c = _pair('covariant', 0, E)
    first = {name: getattr(c['roll']._views(), name).clone() for name in c['roll']._table}
    roll = DeviceRollout(c['ac'], FORMULAS, E, STEPS, gamma=GAMMA, lam=LAM, min_reward=MIN_REWARD, reward_fn=reward_fn,
                         min_atomic_distance=MIN_D, max_solo_distance=MAX_SOLO)
    with torch.no_grad():
        roll.collect(STEPS, seed=SEED + 1)  # another rollout first: the store and the environments are used
        roll.reset()
        with pytest.raises(RuntimeError, match='collect'):
            roll.train_data()
        info = roll.collect(STEPS, seed=SEED)
    assert _same_info(info, c['info'])
    for name, want in first.items():
        assert torch.equal(getattr(roll._views(), name), want), name
    # a shorter collect on a poisoned store: the slots beyond its samples are neither written nor read
    T = 5
    fresh = DeviceRollout(c['ac'], FORMULAS, E, T, gamma=GAMMA, lam=LAM, min_reward=MIN_REWARD, reward_fn=reward_fn,
                          min_atomic_distance=MIN_D, max_solo_distance=MAX_SOLO)
    roll.reset()
    roll.store.fill_(0xFF)
    with torch.no_grad():
        a, b = roll.collect(T, seed=3), fresh.collect(T, seed=3)
    assert _same_info(a, b)
    va, vb = roll._views(), fresh._views()
    for name, (off, dtype, k) in roll._table.items():
        got = getattr(va, name)
        assert got.numel() == E * T * k and torch.equal(got, getattr(vb, name)), name
        if dtype != torch.int32:
            assert not bool(torch.isnan(got).any()), name
        size = 8 if dtype == torch.float64 else 4
        beyond = roll.store[off + E * T * k * size:off + E * STEPS * k * size]
        assert beyond.numel() > 0 and bool((beyond == 0xFF).all()), name
    with pytest.raises(ValueError, match='capacity'):
        fresh.collect(T + 1)


def _mode_pair(ac, E, envs, reward, **kw):
    roll = DeviceRollout(ac, FORMULAS, E, STEPS, gamma=GAMMA, lam=LAM, min_reward=MIN_REWARD, reward_fn=reward,
                         max_solo_distance=MAX_SOLO, **kw)
    with torch.no_grad():
        info = roll.collect(STEPS, seed=SEED)
    box, status, stats = host_rollout(ac, envs, STEPS, SEED)
    hist = _histogram(status)
    assert np.array_equal(roll.statuses(), status)
    assert torch.equal(roll._views().ret, box.merge().get_data(device=ac.theta.device)['ret'])
    assert info['return_mean'] == stats['return_mean'] and info['episode_length_mean'] == stats['episode_length_mean']
    return hist


def test_refills_against_their_host_loop(built_lib):
    E, canvas = 6, 8
    from tests.test_gpu_episodes_env import _agent as agent_of
    ac = agent_of('covariant', 0, ZS, canvas)
    start = tuple(WATER) + ((0, (0.0, 0.0, 0.0)), ) * (canvas - 3)
    envs = [PayingEnvX(canvas, ZS, BAGS, 1.0, MAX_SOLO, start=WATER, num_refills=1) for _ in range(E)]
    hist = _mode_pair(ac, E, envs, reward_fn, initial=(start, BAGS[0]), min_atomic_distance=1.0, num_refills=1)
    assert hist[X.REFILLED] > 0 and sum(hist[s] for s in J.ENDS) > 0, hist


def test_water_start_against_its_host_loop(built_lib):
    E = 6
    ac = _agent('covariant', 2)
    start = tuple(WATER) + ((0, (0.0, 0.0, 0.0)), ) * (CANVAS - 3)
    envs = [PayingEnv(CANVAS, ZS, BAGS, 1.0, MAX_SOLO, start=WATER) for _ in range(E)]
    hist = _mode_pair(ac, E, envs, reward_fn, initial=(start, BAGS[0]), min_atomic_distance=1.0)
    assert hist[J.PLACED] > 0 and sum(hist[s] for s in J.ENDS) > 0, hist


def test_sampled_formulas_without_a_reward_function(built_lib):
    """size_range with reward_fn=None runs: nothing is ever cut, every reward is 0 or min_reward"""
    E = 6
    ac = _agent('covariant', 0)
    roll = DeviceRollout(ac, [((6, 1), (1, 4), (8, 1))], E, STEPS, gamma=GAMMA, lam=LAM, min_reward=MIN_REWARD, min_atomic_distance=1.0,
                         size_range=(2, 5), formula_seed=321)
    with torch.no_grad():
        info = roll.collect(STEPS, seed=SEED)
    status, rew = roll.statuses(), roll._views().rew.cpu().numpy().reshape(E, STEPS)
    hist = _histogram(status)
    assert hist[J.LOW_REWARD] == 0 and hist[J.ERROR] == 0 and hist[J.INACTIVE] == 0
    invalid = np.isin(status, (J.TOO_CLOSE, J.SOLO))
    assert np.all(rew[invalid] == MIN_REWARD) and np.all(rew[~invalid] == 0.0) and invalid.any() and (~invalid).any()
    returns, lengths = rollout.episode_statistics(status, rollout.discounted_returns(status, rew, GAMMA))
    assert len(lengths) == int(np.isin(status, J.ENDS).sum()) > 0 and info['episode_length_mean'] == np.mean(lengths).item()
    assert info['return_mean'] == np.mean(returns).item()
    with pytest.raises(ValueError, match='size_range'):
        DeviceRollout(ac, [((6, 1), (1, 4), (8, 1))], E, STEPS, reward_fn=reward_fn, size_range=(2, 5))


def test_episode_cut_alone(built_lib):
    """rows 1 and 3 of 5 flagged: those two equal a fresh reset with the next formula, the other three are untouched"""
    E = 5
    ac = _agent('covariant', 0)
    roll = DeviceRollout(ac, FORMULAS, E, 2, min_reward=MIN_REWARD, min_atomic_distance=MIN_D)
    cv = roll.canvas
    rng = np.random.RandomState(0)
    pos = torch.from_numpy(rng.normal(size=(E, CANVAS, 3))).cuda()
    pos[:, 2:] = 0.0
    cv.pos64.copy_(pos)
    cv.pos32.copy_(pos.float())
    cv.charges[:, :2] = 6
    cv.natoms_dev.fill_(2)
    cv.bags.copy_(torch.tensor([[0.0, 1.0, 0.0, 1.0]], device='cuda').expand(E, -1))
    roll.episode_no_dev.copy_(torch.tensor([0, 2, 1, 5, 3], dtype=torch.int32))
    v = roll._views(2)
    v.status.fill_(J.PLACED)
    v.rew.fill_(0.125)
    names = ('pos64', 'pos32', 'charges', 'bags', 'natoms_dev')
    before = {k: getattr(cv, k).clone() for k in names}
    before.update(episode_no=roll.episode_no_dev.clone(), status=v.status.clone(), rew=v.rew.clone())
    flags = np.array([0, 1, 0, 1, 0], dtype=np.int32)
    roll._cut(1, 2, v, flags)  # step 1 of 2: slots 1, 3, 5, 7, 9
    torch.cuda.synchronize()
    after = {k: getattr(cv, k) for k in names}
    after.update(episode_no=roll.episode_no_dev, status=v.status, rew=v.rew)
    keep, hit = [0, 2, 4], [1, 3]
    for k in names + ('episode_no', ):
        assert torch.equal(after[k][keep], before[k][keep]), k
    assert torch.equal(cv.pos64[hit], roll._start[0][hit]) and torch.equal(cv.pos32[hit], roll._start[0][hit].float())
    assert torch.equal(cv.charges[hit], roll._start[1][hit]) and torch.equal(cv.natoms_dev[hit], roll._start[2][hit])
    assert after['episode_no'].tolist() == [0, 3, 1, 6, 3]
    assert torch.equal(cv.bags[1], roll._formulas[3 % 2]) and torch.equal(cv.bags[3], roll._formulas[6 % 2])
    want_status, want_rew = before['status'].clone(), before['rew'].clone()
    want_status[[3, 7]], want_rew[[3, 7]] = J.LOW_REWARD, MIN_REWARD
    assert torch.equal(v.status, want_status) and torch.equal(v.rew, want_rew)
    # a row whose step had ended the episode already: only the reward is replaced
    v.status[7] = J.FULL
    v.rew[7] = 0.5
    snapshot = {k: getattr(cv, k).clone() for k in names}
    roll._cut(1, 2, v, np.array([0, 0, 0, 1, 0], dtype=np.int32))
    torch.cuda.synchronize()
    assert all(torch.equal(getattr(cv, k), snapshot[k]) for k in names) and roll.episode_no_dev.tolist() == [0, 3, 1, 6, 3]
    assert int(v.status[7]) == J.FULL and float(v.rew[7]) == MIN_REWARD


def test_bad_arguments_are_refused(built_lib):
    lib, EINVAL = _lib.lib(), -1
    buf = torch.zeros(4096, dtype=torch.float64, device='cuda')
    p = C.c_void_p(buf.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rec = lambda E, T, t, N, Z=4, cols=6, q=p: lib.mg_traj_record(E, T, t, N, Z, cols, p, p, p, p, p, p, p, q, p, p, p, p, p, p, s)
    assert rec(1 << 15, 1 << 10, 0, 64) == EINVAL and b'2^31' in lib.mg_last_error()  # 2^31 elements
    assert rec(2, 3, 3, 4) == EINVAL and rec(2, 3, -1, 4) == EINVAL and rec(0, 3, 0, 4) == EINVAL and rec(2, 0, 0, 4) == EINVAL
    assert rec(2, 3, 0, 256) == EINVAL and rec(2, 3, 0, 4, Z=17) == EINVAL and rec(2, 3, 0, 4, cols=5) == EINVAL
    assert rec(2, 3, 0, 4, q=None) == EINVAL
    assert lib.mg_traj_status(2, 3, 3, p, -0.5, p, p, s) == EINVAL and lib.mg_traj_status(2, 3, 0, None, -0.5, p, p, s) == EINVAL
    assert lib.mg_traj_status(2, 3, 0, p, float('nan'), p, p, s) == EINVAL
    assert lib.mg_traj_gae(2, 0, p, p, p, p, 0.99, 0.95, p, p, p, p, p, s) == EINVAL
    assert lib.mg_traj_gae(2, 3, p, p, p, None, 0.99, 0.95, p, p, p, p, p, s) == EINVAL
    cut = lambda F=1, refills=None, fno=None, flags=p: lib.mg_episode_cut(2, 4, 4, F, 3, 0, flags, -0.5, p, p, p, p, p, p, p, p, p, p, p,
                                                                           refills, fno, p, p, s)
    assert cut(F=0) == EINVAL and cut(refills=p) == EINVAL and cut(fno=p) == EINVAL and cut(flags=None) == EINVAL
    torch.cuda.synchronize()
    assert not bool(buf.any())  # nothing was launched


def _train(ac, data, deterministic):
    import molgym_amd
    ac = copy.deepcopy(ac)
    opt = torch.optim.Adam(ac.parameters(), lr=3e-4)
    np.random.seed(5)
    molgym_amd.set_deterministic(deterministic, covariant=deterministic)
    infos = ppo.train(ac, opt, data, mini_batch_size=36, clip_ratio=0.2, target_kl=1e9, vf_coef=0.5, entropy_coef=0.01, gradient_clip=0.5,
                      max_num_steps=2)
    torch.cuda.synchronize()
    st = opt.state.get(ac.theta, {})
    return infos, ac.theta.detach().clone(), st.get('exp_avg'), st.get('exp_avg_sq')


def test_training_on_the_device_rollout(built_lib):
    """ppo.train on train_data() and on the host loop's data: the same bits in ordered mode, the same statistics without it"""
    c = _pair('covariant', 0, 6)
    a, b = _train(c['ac'], c['roll'].train_data(), True), _train(c['ac'], c['data'], True)
    assert a[0]['num_opt_steps'] == b[0]['num_opt_steps'] == 2 and set(a[0]) == set(b[0])
    for k in a[0]:
        if k != 'time':
            assert a[0][k] == b[0][k], (k, a[0][k], b[0][k])
    assert torch.equal(a[1], b[1]) and not torch.equal(a[1], c['ac'].theta.detach())
    assert a[2] is not None and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    a, b = _train(c['ac'], c['roll'].train_data(), False), _train(c['ac'], c['data'], False)
    assert a[0]['num_opt_steps'] == b[0]['num_opt_steps'] == 2
    for k in ppo.KEYS:
        assert rel_err(torch.tensor(a[0][k]), torch.tensor(b[0][k])) < 1e-5, (k, a[0][k], b[0][k])


def test_schnet_trains_on_its_host_form(built_lib):
    c = _pair('internal', 5, 6)
    data = c['roll'].train_data()
    assert isinstance(data['obs'], list)
    ac = copy.deepcopy(c['ac'])
    infos = ppo.train(ac, torch.optim.Adam(ac.parameters(), lr=3e-4), data, mini_batch_size=36, clip_ratio=0.2, target_kl=1e9, vf_coef=0.5,
                      entropy_coef=0.01, gradient_clip=0.5, max_num_steps=1)
    assert infos['num_opt_steps'] == 1 and np.isfinite(infos['total_loss'])
