"""The host statement of DeviceRollout's store and segmented GAE (tests/traj_ref.py) against the buffers it replaces
(`DynamicPPOBuffer.finish_path`, `PPOBufferContainer.merge()`), the statistics of `collect`, and the refusals.  No GPU."""
import types

import numpy as np
import pytest
import torch

from molgym_amd import ppo, rollout
from molgym_amd.buffer import PPOBufferContainer
from molgym_amd.observations import CarriedRollout
from tests import traj_ref as J

GAMMA, LAM, MIN_REWARD = 0.99, 0.95, -0.6
P, S, C, B, L, F = J.PLACED, J.STOP, J.TOO_CLOSE, J.BAG_EMPTY, J.LOW_REWARD, J.FULL
# per environment the statuses of 6 steps: never terminal; terminal at its last slot; two finished paths and an open tail; a
# cut (LOW_REWARD) and a rule rejection; a row whose every slot ends an episode
TABLE = np.array([[P, P, P, P, P, P],
                  [P, P, P, P, P, B],
                  [P, P, S, P, F, P],
                  [P, P, P, L, C, P],
                  [S, S, C, S, B, L]], dtype=np.int32)


def _fill(table, seed=0):
    """rewards as the store holds them, float32 values / logps widened, bootstrap values"""
    rng = np.random.RandomState(seed)
    E, T = table.shape
    rew = np.zeros((E, T))
    for e in range(E):
        for t in range(T):
            s = int(table[e, t])
            if s == L:
                rew[e, t] = MIN_REWARD
            elif s in J.ATOM:
                rew[e, t] = max(rng.normal(), MIN_REWARD)
            else:
                rew[e, t] = J.rule_reward(s, MIN_REWARD)
    val = rng.normal(size=(E, T)).astype(np.float32)
    logp = rng.normal(size=(E, T)).astype(np.float32)
    last = rng.normal(size=E).astype(np.float32)
    return rew, val, logp, last


def _container(table, rew, val, logp, last):
    """the same steps through PPOBufferContainer, as ppo._rollout_serial feeds it"""
    E, T = table.shape
    box = PPOBufferContainer(size=E, gamma=GAMMA, lam=LAM)
    for t in range(T):
        box.store(observations=[(e, t) for e in range(E)], actions=np.zeros((E, 6), np.float32), rewards=rew[:, t],
                  next_observations=[None] * E, terminals=np.isin(table[:, t], J.ENDS), values=val[:, t], logps=logp[:, t])
    box.finish_paths(last)
    return box


def test_segmented_gae_equals_the_buffers_path_for_path():
    rew, val, logp, last = _fill(TABLE)
    box = _container(TABLE, rew, val, logp, last)
    merged = box.merge()
    E, T = TABLE.shape
    adv, ret, num_done, len_sum, len_sq = J.segmented_gae(TABLE, rew, val.astype(np.float64), last.astype(np.float64), GAMMA, LAM)
    # sample e * T + t is the merged buffer's order
    assert merged.obs_buf == [(e, t) for e in range(E) for t in range(T)]
    assert np.array_equal(adv.reshape(-1), np.array(merged.adv_buf)) and np.array_equal(ret.reshape(-1), np.array(merged.ret_buf))
    for lo, hi, lv in merged.paths:  # path for path: ends where a status ends it, bootstraps only the open tails
        e, t1 = divmod(hi - 1, T)
        ended = int(TABLE[e, t1]) in J.ENDS
        assert ended or t1 == T - 1
        assert lv == (0.0 if ended else float(last[e]))
        assert lo == e * T or int(TABLE[e, lo - e * T - 1]) in J.ENDS
        assert not np.isin(TABLE[e, lo - e * T:t1], J.ENDS).any()
    assert [len(b.paths) for b in box.buffers] == [1, 1, 3, 3, 6]
    # the normalised advantages of get_data()
    assert np.array_equal(J.normalize(adv.reshape(-1)), merged.get_data()['adv'])
    # the statistics: counts, length sums, and the lists in the container's order (by step, then environment)
    returns, lengths = rollout.episode_statistics(TABLE, ret)
    assert np.array_equal(returns, np.array(box.episodic_returns)) and list(lengths) == box.episode_lengths
    host_returns = rollout.episode_statistics(TABLE, rollout.discounted_returns(TABLE, rew, GAMMA))[0]  # (what collect reports)
    assert np.array_equal(host_returns, np.array(box.episodic_returns))
    assert int(num_done.sum()) == len(box.episode_lengths) and list(num_done) == [0, 1, 2, 2, 6]
    assert len_sum.sum() == sum(box.episode_lengths) and len_sq.sum() == sum(n * n for n in box.episode_lengths)
    assert len_sum.sum() / num_done.sum() == np.mean(box.episode_lengths)


def test_store_restates_the_steps_and_the_cut():
    """record / status / rewards of the host store: the slot order, the widening, the rule rewards and the cut"""
    E, T, N, Z = 3, 2, 4, 3
    st = J.TrajStore(E, T, N, Z, 6)
    rng = np.random.RandomState(1)
    pos = rng.normal(size=(E, N, 3))
    logp, v = rng.normal(size=E).astype(np.float32), rng.normal(size=E).astype(np.float32)
    acts = rng.normal(size=(E, 6)).astype(np.float32)
    st.record(1, pos, np.ones((E, N), np.int32), np.ones((E, Z), np.float32), acts, logp, v, alive=[1, 0, 1])
    st.set_status(1, np.array([P, J.INACTIVE, J.SOLO]), MIN_REWARD)
    assert np.array_equal(st.pos64[1], pos[0]) and np.array_equal(st.pos[5], pos[2].astype(np.float32))
    assert not st.pos64[3].any() and not st.pos64[0].any()  # the stopped row and step 0 wrote nothing
    assert st.logp[1] == float(logp[0]) and st.val[5] == float(v[2]) and st.logp.dtype == np.float64
    assert st.rew[5] == MIN_REWARD and st.rew[1] == 0.0 and list(st.status) == [0, P, 0, 0, 0, J.SOLO]
    assert st.set_rewards(1, [0], [MIN_REWARD - 0.1], MIN_REWARD) == [0] and st.status[1] == L and st.rew[1] == MIN_REWARD
    assert J.pay(F, -5.0, MIN_REWARD) == (F, MIN_REWARD) and J.pay(B, 0.25, MIN_REWARD) == (B, 0.25)
    assert J.pay(J.REFILLED, -5.0, MIN_REWARD) == (L, MIN_REWARD) and J.pay(P, MIN_REWARD, MIN_REWARD) == (P, MIN_REWARD)


def _stub(zs, canvas_size):
    return types.SimpleNamespace(zs=list(zs), theta=types.SimpleNamespace(device=types.SimpleNamespace(type='cpu')),
                                 observation_space=types.SimpleNamespace(canvas_space=types.SimpleNamespace(size=canvas_size)))


def test_refusals_without_a_device(monkeypatch):
    ac = _stub([0, 1, 6, 8], 6)
    formulas = [((6, 1), (1, 4), (8, 1))]
    with pytest.raises(ValueError, match='capacity'):
        rollout.DeviceRollout(ac, formulas, 4, 0)
    with pytest.raises(ValueError, match='size_range'):
        rollout.DeviceRollout(ac, formulas, 4, 8, reward_fn=lambda *a: np.zeros(len(a[3])), size_range=(2, 5))
    with pytest.raises(ValueError, match='2\\^31'):
        rollout.DeviceRollout(ac, formulas, 1 << 20, 1 << 10)
    # what passes these checks reaches DeviceEpisodes' own (size_range without a reward function is allowed)
    with pytest.raises(RuntimeError, match='HIP device only'):
        rollout.DeviceRollout(ac, formulas, 4, 8, size_range=(2, 5))
    with pytest.raises(RuntimeError, match='HIP device only'):
        rollout.DeviceRollout(ac, formulas, 4, 8, reward_fn=lambda *a: np.zeros(len(a[3])))
    # num_steps beyond the capacity is refused before anything else is touched
    bare = object.__new__(rollout.DeviceRollout)
    bare.capacity = 4
    for bad in (5, 0):
        with pytest.raises(ValueError, match='capacity'):
            bare.collect(bad)
    # ppo.train at world size > 1
    data = dict(obs=CarriedRollout(12, object()), act=None, ret=None, adv=None, logp=None)
    monkeypatch.setattr(ppo, '_dist', lambda: (object(), 0, 2))
    with pytest.raises(RuntimeError, match='world size 2'):
        ppo.train(None, None, data, 4, 0.2, 0.01, 0.5, 0.01, 0.5, 2)


def test_carried_rollout_is_handed_back():
    from molgym_amd.agents.covariant import CovariantAC
    marker = object()
    carrier = CarriedRollout(140, marker)
    assert len(carrier) == 140 and carrier.rollout is marker
    with pytest.raises(TypeError):
        carrier[0]
    assert CovariantAC.prepare_rollout(None, {'obs': carrier}) is marker
    assert rollout.STATUS_NAMES[J.LOW_REWARD] == 'LOW_REWARD' and len(rollout.STATUS_NAMES) == 11
    assert J.LOW_REWARD in rollout.END_STATUSES and J.PLACED not in rollout.END_STATUSES and J.REFILLED not in rollout.END_STATUSES


def test_store_layout_is_aligned_and_disjoint():
    table, total = rollout.store_layout(5, 7, 6, 4, 6)
    S, spans = 35, []
    for name, (off, dtype, k) in table.items():
        size = 8 if dtype == torch.float64 else 4
        assert off % 256 == 0, name
        spans.append((off, off + S * k * size))
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= total < spans[-1][1] + 256
