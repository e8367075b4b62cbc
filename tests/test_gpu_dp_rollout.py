"""Device rollouts under data parallelism: `DeviceRollout(..., shard=(rank, world))`, `mg_traj_pack` / `mg_traj_unpack` and the
gathered rollout `train_data()` hands `ppo.train` (molgym_amd/rollout.py).

* the two kernels through the C ABI against the numpy mirror of tests/exchange_ref.py, every byte, between guard bands;
* a shard against its host loop -- `host_rollout` of tests/test_gpu_device_rollout.py on the shard's environments, keyed by their
  global numbers: `step_canvas(..., sample_ids=(lo, 1))`, `draw_key = (seed, lo + e)`.  Both sides run at the shard's batch.
  `SHARD_T` = 8 steps in a store of capacity 24 (the `STEPS` of that test).  At T = 4 the world-1 host loop of all 5
  environments meets the not-vacuous condition for both agents, but the environments 0..2 that the shards (1, 3) and (0, 2) cover
  meet no rule rejection in 4 steps; 8 is the shortest collect at which both the 5 and those 3 meet it, for both agents;
* worlds 2 and 3 emulated in one process: the shards' blocks stacked as the collective stacks them, `unpack_gathered` on every rank;
* world invariance: the gathered rollout equals the collect of one process, array by array.  It stands on the sampling launch
  giving a row the same bits at batch 5 and at batches 1, 2, 3, which tools/dp_rollout_probe.py found bit-equal for both agents
  (profiles/dp_device_rollout.md);
* two real ranks over gloo on device 0: gathered bytes and the ordered data-parallel update against the in-process emulation."""
import ctypes as C
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from molgym_amd import _lib, ppo, rollout
from molgym_amd.buffer import PPOBufferContainer
from molgym_amd.rollout import DeviceRollout, _Views
from tests import exchange_ref as X
from tests import traj_ref as J
from tests.dp_rollout_worker import AGENT_SEED, CAPACITY, NUM_ENVS, T, gathered_arrays, make_rollout, train
from tests.test_gpu_device_rollout import GAMMA, LAM, MIN_REWARD, SEED, PayingEnv, _seeds, reward_fn
from tests.test_gpu_episodes import BAGS, CANVAS, FORMULAS, MAX_SOLO, MIN_D, STEPS, ZS, _agent

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096
# the shortest collect at which the world-1 host loop of 5 environments AND its rows 0..2 (what the shards (1, 3) and (0, 2)
# cover) meet the not-vacuous condition for both agents (module docstring); the stores have the capacity STEPS = 24
SHARD_T = 8
KINDS = ['covariant', 'internal']
CHILD_TIMEOUT = 300.0  # cold start of two children (import, device, library, process group) + one collect and a 3-epoch train


@pytest.fixture(autouse=True)
def _restore_switches(built_lib):
    prev = (_lib.is_deterministic(), _lib.is_deterministic_covariant(), _lib.is_deterministic_data_parallel())
    yield
    _lib.set_deterministic(prev[0], covariant=prev[1], data_parallel=prev[2])


_AGENTS = {}


def _ac(kind):
    if kind not in _AGENTS:
        _AGENTS[kind] = _agent(kind, AGENT_SEED[kind])
    return _AGENTS[kind]


# ---- the kernels against the numpy mirror ---------------------------------------------------------------------------------------
def _guarded(nbytes, byte):
    big = torch.full((GUARD + nbytes + GUARD, ), 0xA5, dtype=torch.uint8, device='cuda')
    big[GUARD:GUARD + nbytes].fill_(byte)
    return big, big[GUARD:GUARD + nbytes]


def _guards_intact(big, nbytes):
    return bool((big[:GUARD] == 0xA5).all()) and bool((big[GUARD + nbytes:] == 0xA5).all())


def _abi(num_envs, world, T_, N, Z, cols):
    sections, block_bytes = rollout.exchange_layout(num_envs, world, T_, N, Z, cols)
    off = (C.c_int64 * len(sections))(*[o for o, _, _ in sections.values()])
    words = (C.c_int32 * len(sections))(*[k * (2 if dtype == torch.float64 else 1) for _, dtype, k in sections.values()])
    return sections, block_bytes, off, words


def _pointers(sections, table, store, natoms):
    """the 12 device pointers of a store's arrays and its atom counts, in section order"""
    return (C.c_void_p * len(sections))(*[natoms.data_ptr() if name == 'natoms' else store.data_ptr() + table[name][0] for name in sections])


EXCHANGE_CASES = [(6, 4, 6, 5, 3, 4, 6), (6, 4, 7, 5, 2, 4, 6), (255, 16, 7, 3, 2, 1, 2), (7, 3, 6, 70, 3, 3, 3)]


@pytest.mark.parametrize('byte', [0xFF, 0x7F])
@pytest.mark.parametrize('N,Z,cols,num_envs,world,T_,capacity', EXCHANGE_CASES)
def test_pack_and_unpack_against_the_numpy_mirror(built_lib, N, Z, cols, num_envs, world, T_, capacity, byte):
    lib, s = _lib.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(1000 * N + num_envs)
    sections, block_bytes, off, words = _abi(num_envs, world, T_, N, Z, cols)
    shares = [rollout.shard_bounds(num_envs, r, world) for r in range(world)]
    blocks = []
    for r, (lo, hi) in enumerate(shares):
        host_store = X.random_store(rng, hi - lo, capacity, N, Z, cols)
        host_natoms = rng.integers(0, N, size=(hi - lo) * T_).astype(np.int32)
        store, natoms = torch.from_numpy(host_store).cuda(), torch.from_numpy(host_natoms).cuda()
        big, block = _guarded(block_bytes, byte)
        table = rollout.store_layout(hi - lo, capacity, N, Z, cols)[0]
        rc = lib.mg_traj_pack(num_envs, world, r, T_, capacity, N, len(sections), off, words, _pointers(sections, table, store, natoms),
                              C.c_void_p(block.data_ptr()), block_bytes, s)
        assert rc == 0, lib.mg_last_error()
        torch.cuda.synchronize()
        want = X.pack(host_store, host_natoms, num_envs, world, r, T_, capacity, N, Z, cols, block=np.full(block_bytes, byte, dtype=np.uint8))
        assert _guards_intact(big, block_bytes), r
        assert np.array_equal(block.cpu().numpy(), want), r  # (every byte: the padding and a short share's tail stay poisoned)
        assert np.array_equal(store.cpu().numpy(), host_store)
        blocks.append(want)
    assert len({hi - lo for lo, hi in shares}) > 1  # a short share is among them
    gathered = np.stack(blocks)
    gtable, nbytes = rollout.store_layout(num_envs, capacity, N, Z, cols)
    big, gstore = _guarded(nbytes, byte)
    big_n, gnatoms = _guarded(4 * num_envs * T_, byte)
    rc = lib.mg_traj_unpack(num_envs, world, T_, capacity, N, len(sections), off, words, C.c_void_p(torch.from_numpy(gathered).cuda().data_ptr()),
                            block_bytes, _pointers(sections, gtable, gstore, gnatoms), s)
    assert rc == 0, lib.mg_last_error()
    torch.cuda.synchronize()
    want_store, want_natoms = X.unpack(gathered, num_envs, world, T_, capacity, N, Z, cols, store=np.full(nbytes, byte, dtype=np.uint8),
                                       natoms=np.frombuffer(bytes([byte]) * (4 * num_envs * T_), dtype=np.int32).copy())
    assert _guards_intact(big, nbytes) and _guards_intact(big_n, 4 * num_envs * T_)
    assert np.array_equal(gstore.cpu().numpy(), want_store)
    assert np.array_equal(gnatoms.cpu().numpy().view(np.int32), want_natoms)
    if T_ < capacity:  # the used part of a store is not its whole: something stayed poisoned
        assert (want_store == byte).sum() > nbytes // 4


def test_exchange_refusals(built_lib):
    lib, EINVAL = _lib.lib(), -1
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    N, Z, cols, num_envs, world, T_, capacity = EXCHANGE_CASES[0]
    sections, block_bytes, off, words = _abi(num_envs, world, T_, N, Z, cols)
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device='cuda')
    p = C.c_void_p(buf.data_ptr())
    arrays = (C.c_void_p * 12)(*[buf.data_ptr()] * 12)
    pack = lambda T__=T_, cap=capacity, block=p, arr=arrays, envs=num_envs, w=world, r=0, n=N, nsec=12, bb=block_bytes: \
        lib.mg_traj_pack(envs, w, r, T__, cap, n, nsec, off, words, arr, block, bb, s)
    unpack = lambda T__=T_, cap=capacity, src=p, arr=arrays, envs=num_envs, w=world, n=N, bb=block_bytes: \
        lib.mg_traj_unpack(envs, w, T__, cap, n, 12, off, words, src, bb, arr, s)
    assert pack(T__=capacity + 1) == EINVAL and b'capacity' in lib.mg_last_error()
    assert unpack(T__=capacity + 1) == EINVAL and b'capacity' in lib.mg_last_error()
    assert pack(block=None) == EINVAL and b'null' in lib.mg_last_error()
    assert unpack(src=None) == EINVAL and pack(arr=None) == EINVAL and unpack(arr=None) == EINVAL
    holed = (C.c_void_p * 12)(*([buf.data_ptr()] * 11 + [None]))
    assert pack(arr=holed) == EINVAL and unpack(arr=holed) == EINVAL
    # a gathered store of 2^31 elements: 2^15 environments x 2^10 steps x 64 atoms x 3
    assert pack(T__=1, cap=1 << 10, envs=1 << 15, n=64) == EINVAL and b'2^31' in lib.mg_last_error()
    assert unpack(T__=1, cap=1 << 10, envs=1 << 15, n=64) == EINVAL and b'2^31' in lib.mg_last_error()
    assert pack(r=world) == EINVAL and pack(r=-1) == EINVAL and pack(w=0) == EINVAL and pack(envs=2) == EINVAL and pack(nsec=11) == EINVAL
    assert pack(T__=0) == EINVAL and pack(n=256) == EINVAL and unpack(w=num_envs + 1) == EINVAL
    assert pack(bb=block_bytes - 256) == EINVAL and unpack(bb=block_bytes - 256) == EINVAL  # the last section runs past the block
    torch.cuda.synchronize()
    assert not bool(buf.any())  # nothing was launched


# ---- a shard against its host loop ----------------------------------------------------------------------------------------------
def shard_host_rollout(ac, lo, hi, T_, seed):
    """`host_rollout` of tests/test_gpu_device_rollout.py on the environments lo..hi-1, keyed by their global numbers"""
    envs = [PayingEnv(CANVAS, ZS, BAGS, MIN_D, MAX_SOLO) for _ in range(lo, hi)]
    E = len(envs)
    box = PPOBufferContainer(size=E, gamma=GAMMA, lam=LAM)
    seeds = _seeds(seed, T_)
    obs = [env._obs() for env in envs]
    cv = ac.make_canvas(obs)
    status = np.zeros((E, T_), dtype=np.int32)
    with torch.no_grad():
        for t in range(T_):
            pred = ac.step_canvas(cv, seed=seeds[t], sample_ids=(lo, 1))
            nxt, rewards, terminals = [], [], []
            for e, env in enumerate(envs):
                env.draw_key = (seeds[t], lo + e)
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
        last = ac.step_canvas(cv, commit=False, seed=seeds[T_], sample_ids=(lo, 1))
        box.finish_paths(ppo._host_predictions(last)[1])
    stats = dict(return_mean=np.mean(box.episodic_returns).item(), return_std=np.std(box.episodic_returns).item(),
                 episode_length_mean=np.mean(box.episode_lengths).item(), episode_length_std=np.std(box.episode_lengths).item())
    return box, status, stats


def host_raw_advantages(merged, dev):
    """the host loop's RAW advantages as its device form evaluates them: `DynamicPPOBuffer.get_data(device=...)` without its last
    step, the standardisation -- `mg_gae` over the buffer's own rewards, values and paths (the kernel whose recursion
    `mg_traj_gae` shares: gae_step, csrc/ppo.inc).  `get_data(device=...)` is where the existing test takes `ret` from."""
    T_, P = merged.current_index, len(merged.paths)
    off = np.array([p[0] for p in merged.paths] + [T_], dtype=np.int32)
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    rew, val = up(merged.rew_buf, np.float64), up(merged.val_buf, np.float64)
    last, d_off = up([p[2] for p in merged.paths], np.float64), up(off, np.int32)
    adv, ret = torch.empty(T_, dtype=torch.float64, device=dev), torch.empty(T_, dtype=torch.float64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(_lib.lib().mg_gae(P, p(d_off), p(rew), p(val), p(last), float(merged.gamma), float(merged.lam), p(adv), p(ret),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return adv


_SHARD_STATUS = {}


@pytest.mark.parametrize('shard', [(1, 3), (0, 2)])
@pytest.mark.parametrize('kind', KINDS)
def test_shard_equals_its_host_loop(built_lib, kind, shard):
    ac = _ac(kind)
    lo, hi = rollout.shard_bounds(NUM_ENVS, *shard)
    seen = []

    def recording_reward(before, new_z, new_pos, rows):
        seen.extend(int(r) for r in rows)
        return reward_fn(before, new_z, new_pos, rows)

    roll = make_rollout(ac, shard, recording_reward, capacity=STEPS)
    assert (roll.E, roll.num_envs, roll.lo, roll.hi) == (hi - lo, NUM_ENVS, lo, hi)
    with torch.no_grad():
        info = roll.collect(SHARD_T, seed=SEED)
    box, status, stats = shard_host_rollout(ac, lo, hi, SHARD_T, SEED)
    merged = box.merge()
    assert seen and set(seen) <= set(range(lo, hi))  # the reward function saw global environment numbers
    assert np.array_equal(roll.statuses(), status)
    for k in stats:
        assert info[k] == stats[k] or (np.isnan(info[k]) and np.isnan(stats[k])), (k, info[k], stats[k])
    v, S = roll._views(), (hi - lo) * SHARD_T
    dev = ac.theta.device
    data = merged.get_data(device=dev)  # (the host loop's data of the existing test: logp uploaded, ret from mg_gae)
    want = {'logp': data['logp'], 'ret': data['ret'], 'adv': host_raw_advantages(merged, dev)}  # adv: the RAW advantages
    for k, w in want.items():
        got = getattr(v, k)
        print(kind, shard, k, 'max |diff|', float((got - w).abs().max()))
        assert got.dtype == torch.float64 and torch.equal(got, w), k
    # and against the float64 numpy buffers of the host loop, at the tolerance the existing GAE test holds the store to: the
    # kernels contract r + gamma * v into one rounding, numpy rounds twice (measured on the covariant shard (1, 3): 2.8e-17)
    np.testing.assert_allclose(v.adv.cpu().numpy(), np.array(merged.adv_buf), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(v.ret.cpu().numpy(), np.array(merged.ret_buf), rtol=1e-12, atol=1e-14)
    # positions (float64), charges and bags: the observation tuples rebuilt from the store; the action rows
    host = roll.data()
    assert len(host['obs']) == S == len(merged.obs_buf)
    for s_, (a, b) in enumerate(zip(host['obs'], merged.obs_buf)):
        assert a == b, s_
    assert np.array_equal(host['act'], np.array(merged.act_buf)) and host['act'].dtype == np.float32
    assert torch.equal(v.actions.view(S, roll.cols).cpu(), torch.from_numpy(host['act']))
    if kind == 'covariant':  # the float32 arrays of RolloutOnDevice as prepare_rollout parses them from the host loop's data
        parsed = ac.prepare_rollout(merged.get_data(device=dev))
        for name, a, b in zip(('pos', 'charges', 'bags', 'actions'), (v.pos.view(S, CANVAS, 3), v.charges.view(S, CANVAS),
                                                                      v.bags.view(S, len(ZS)), v.actions.view(S, 6)), parsed.t):
            assert a.dtype == b.dtype and torch.equal(a, b), name
        assert np.array_equal(roll._natoms_hist.reshape(-1), parsed.natoms)
    _SHARD_STATUS[(kind, shard)] = status
    both = [_SHARD_STATUS.get((kind, sh)) for sh in ((1, 3), (0, 2))]
    if all(b is not None for b in both):  # not vacuous on the union of the shards (the condition of the existing test)
        hist = sum(np.bincount(b.reshape(-1), minlength=11) for b in both)
        print('statuses:', {rollout.STATUS_NAMES[i]: int(n) for i, n in enumerate(hist) if n})
        assert hist[J.PLACED] > 0 and hist[J.BAG_EMPTY] + hist[J.FULL] > 0 and hist[J.TOO_CLOSE] + hist[J.SOLO] > 0, hist
        assert hist[J.LOW_REWARD] > 0 and sum(int((~np.isin(b[:, -1], J.ENDS)).sum()) for b in both) > 0, hist
        assert hist[J.ERROR] == 0 and hist[J.INACTIVE] == 0


# ---- worlds emulated in one process ---------------------------------------------------------------------------------------------
_WORLDS = {}


def _emulated(kind, world):
    """the shards of `world` collected one after another on one agent with one seed, their blocks stacked as the collective would
    stack them, and `unpack_gathered` on every rank (shared by the tests that read it; nothing is changed afterwards)"""
    if (kind, world) not in _WORLDS:
        ac = _ac(kind)
        rolls = [make_rollout(ac, (r, world), reward_fn) for r in range(world)]
        raw, blocks = [], []
        with torch.no_grad():
            for roll in rolls:
                roll.collect(T, seed=SEED)
                raw.append(roll._views().adv.clone())
                blocks.append(roll.pack().clone())
        stacked = torch.cat(blocks)
        data = [roll.unpack_gathered(stacked, T, on_device=True) for roll in rolls]
        torch.cuda.synchronize()
        _WORLDS[(kind, world)] = dict(ac=ac, rolls=rolls, raw=torch.cat(raw).cpu().numpy(), data=data)
    return _WORLDS[(kind, world)]


def _straddling(world):
    """sample indices on both sides of every share boundary, and the two ends of the rollout"""
    idx = [0, NUM_ENVS * T - 1]
    for r in range(1, world):
        b = rollout.shard_bounds(NUM_ENVS, r, world)[0] * T
        idx += [b - 2, b - 1, b, b + 1]
    return np.array(idx, dtype=np.int64)


def _one_minibatch(ac, prepared, idx):
    ac.theta.grad = torch.zeros_like(ac.theta)
    ac.invalidate_weights()
    stats = ac.ppo_minibatch(prepared.minibatch(idx), 0.2, 0.5, 0.01)
    if hasattr(ac, 'fold_gradients'):
        ac.fold_gradients()
    torch.cuda.synchronize()
    assert stats is not None and bool(torch.isfinite(stats).all()), stats
    assert bool(torch.isfinite(ac.theta.grad).all()) and ac.theta.grad.abs().max().item() > 0
    ac.theta.grad = None


@pytest.mark.parametrize('world', [2, 3])
@pytest.mark.parametrize('kind', KINDS)
def test_emulated_world_gathers_one_rollout(built_lib, kind, world):
    c = _emulated(kind, world)
    ac, rolls, S = c['ac'], c['rolls'], NUM_ENVS * T
    first = gathered_arrays(rolls[0])
    for r, roll in enumerate(rolls):
        assert roll._gstore.data_ptr() != rolls[0]._gstore.data_ptr() or r == 0
        mine = gathered_arrays(roll)
        for name in first:
            assert mine[name].dtype == first[name].dtype and torch.equal(mine[name].view(torch.uint8), first[name].view(torch.uint8)), (r, name)
    # the advantages: the standardisation of buffer.py:104-110 over the gathered RAW ones, at the tolerance of the existing GAE test
    np.testing.assert_allclose(first['adv'].numpy(), J.normalize(c['raw']), rtol=1e-11, atol=1e-13)
    assert np.array_equal(first['natoms'].numpy(), np.concatenate([roll._natoms_hist.reshape(-1) for roll in rolls]))
    idx = _straddling(world)
    for roll, data in zip(rolls, c['data']):
        assert data['obs'].world == world and len(data['obs']) == S
        prepared = ac.prepare_rollout(data)
        assert prepared is data['obs'].rollout and np.array_equal(prepared.natoms, first['natoms'].numpy())
        assert data['adv'].shape == (S, ) and data['act'].shape == (S, roll.cols)
    _one_minibatch(ac, c['data'][-1]['obs'].rollout, idx)
    if kind == 'internal':  # SchNetAC's other form: the host form of the GATHERED store (cached: no collective)
        host = rolls[0].train_data()
        assert isinstance(host['obs'], list) and len(host['obs']) == S and torch.equal(host['adv'].cpu(), first['adv'])
        _one_minibatch(ac, ac.prepare_rollout(host), idx)
    else:
        assert rolls[0].train_data()['obs'].rollout.t[0].data_ptr() == c['data'][0]['obs'].rollout.t[0].data_ptr()


_SINGLE = {}


def _single(kind):
    if kind not in _SINGLE:
        roll = make_rollout(_ac(kind), None, reward_fn)
        with torch.no_grad():
            info = roll.collect(T, seed=SEED)
        _SINGLE[kind] = (roll, info, roll.train_data(on_device=True))
    return _SINGLE[kind]


@pytest.mark.parametrize('world', [2, 3])
@pytest.mark.parametrize('kind', KINDS)
def test_world_invariance(built_lib, kind, world):
    """the gathered rollout IS the collect of one process driving all 5 environments (tools/dp_rollout_probe.py: the sampling
    launch gives a row the same bits at every batch these shards have, for both agents)"""
    roll, _, data = _single(kind)
    assert data['obs'].world == 1
    got = gathered_arrays(_emulated(kind, world)['rolls'][0])
    v = roll._views()
    for name in roll._table:
        a, b = getattr(v, name).cpu(), got[name]
        assert a.shape == b.shape and torch.equal(a, b), name
    assert np.array_equal(roll._natoms_hist.reshape(-1), got['natoms'].numpy())
    assert np.array_equal(roll.statuses(), np.concatenate([r.statuses() for r in _emulated(kind, world)['rolls']]))


def test_sampled_formulas_follow_the_global_streams(built_lib):
    """size_range, reward_fn=None: the bags a shard draws at reset() and at episode ends are rows lo..hi of the unsharded draws"""
    ac = _ac('covariant')
    kw = dict(gamma=GAMMA, lam=LAM, min_reward=MIN_REWARD, min_atomic_distance=1.0, size_range=(2, 5), formula_seed=321)
    formula = [((6, 1), (1, 4), (8, 1))]
    full = DeviceRollout(ac, formula, NUM_ENVS, STEPS, **kw)
    start = full.canvas.bags.clone()
    assert len({tuple(b) for b in start.cpu().tolist()}) > 1  # the environments did not all draw one formula
    with torch.no_grad():
        full.collect(STEPS, seed=SEED)
    bags = full._views().bags.view(NUM_ENVS, STEPS, len(ZS))
    ends = np.isin(full.statuses(), J.ENDS)
    for world in (2, 3):
        for r in range(world):
            lo, hi = rollout.shard_bounds(NUM_ENVS, r, world)
            part = DeviceRollout(ac, formula, NUM_ENVS, STEPS, shard=(r, world), **kw)
            assert torch.equal(part.canvas.bags, start[lo:hi]), (world, r)
            with torch.no_grad():
                part.collect(STEPS, seed=SEED)
            assert np.array_equal(part.statuses(), full.statuses()[lo:hi]), (world, r)
            assert torch.equal(part._views().bags.view(hi - lo, STEPS, len(ZS)), bags[lo:hi]), (world, r)
            assert torch.equal(part.canvas.bags, full.canvas.bags[lo:hi])
            assert ends[lo:hi, :-1].any(), (world, r)  # an episode ended in this share: a draw behind reset() was compared


@pytest.mark.parametrize('kind', KINDS)
def test_sharded_episodes_carry_global_numbers(built_lib, kind):
    """`DeviceEpisodes(shard=...)`: the finished episodes of a share are those of its environments in the unsharded run, under
    their global numbers (world invariance of the sampling launch, as above)"""
    from molgym_amd.episodes import DeviceEpisodes
    ac = _ac(kind)
    whole = DeviceEpisodes(ac, FORMULAS, NUM_ENVS, min_atomic_distance=MIN_D, max_solo_distance=MAX_SOLO).run(num_steps=SHARD_T, seed=5)
    assert len(whole) > 0
    for shard in ((1, 3), (2, 3), (0, 2)):
        lo, hi = rollout.shard_bounds(NUM_ENVS, *shard)
        part = DeviceEpisodes(ac, FORMULAS, NUM_ENVS, min_atomic_distance=MIN_D, max_solo_distance=MAX_SOLO, shard=shard)
        assert (part.E, part.num_envs) == (hi - lo, NUM_ENVS)
        got, want = part.run(num_steps=SHARD_T, seed=5), [ep for ep in whole if lo <= ep.env < hi]
        assert len(got) == len(want) > 0
        for a, b in zip(got, want):
            assert (a.env, a.formula, a.status) == (b.env, b.formula, b.status)
            assert np.array_equal(a.numbers, b.numbers) and np.array_equal(a.positions, b.positions) and np.array_equal(a.logp, b.logp)
    with pytest.raises(ValueError, match='rank'):
        DeviceEpisodes(ac, FORMULAS, NUM_ENVS, shard=(3, 3))
    with pytest.raises(ValueError, match='environments'):
        DeviceEpisodes(ac, FORMULAS, 2, shard=(0, 3))


def test_default_shard_changes_nothing(built_lib):
    """shard=None, (0, 1) and the unsharded call of before: the same store"""
    roll, info, _ = _single('covariant')
    other = make_rollout(_ac('covariant'), (0, 1), reward_fn)
    with torch.no_grad():
        other.collect(T, seed=SEED)
    assert other.store_bytes == roll.store_bytes == rollout.store_layout(NUM_ENVS, CAPACITY, CANVAS, len(ZS), 6)[1]
    for name in roll._table:
        assert torch.equal(getattr(roll._views(), name), getattr(other._views(), name)), name
    # pack / unpack at world 1 is the identity on the used part of the store
    data = other.unpack_gathered(other.pack(), T, on_device=True)
    got = gathered_arrays(other)
    for name in roll._table:
        if name != 'adv':  # (standardised a second time by unpack_gathered: not the same map)
            assert torch.equal(getattr(roll._views(), name).cpu(), got[name]), name
    assert data['obs'].world == 1


# ---- a real process group -------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _run_world(kind, world, tmp_path):
    """the ranks as child processes under ONE time limit; on a time-out or a non-zero exit every child is killed and reaped before
    the assertion fires; nothing is retried (the structure of tests/test_gpu_dp_ordered.py::_run_world)"""
    port, tag = _free_port(), f'{kind}.w{world}'
    outs = [str(tmp_path / f'{tag}.r{r}.pt') for r in range(world)]
    logs = [open(str(tmp_path / f'{tag}.r{r}.log'), 'w') for r in range(world)]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    for k in ('MG_DETERMINISTIC', 'MG_COV_ORDERED', 'MG_DP_ORDERED', 'MOLGYM_RUNAHEAD'):
        env.pop(k, None)
    start = time.time()
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, 'tests', 'dp_rollout_worker.py'), kind, str(r), str(world), str(port), outs[r]],
                              cwd=ROOT, env=env, stdout=logs[r], stderr=subprocess.STDOUT) for r in range(world)]
    failure = None
    try:
        while failure is None:
            codes = [p.poll() for p in procs]
            if any(c not in (None, 0) for c in codes):
                failure = f'exit codes {codes}'
            elif all(c == 0 for c in codes):
                break
            elif time.time() - start > CHILD_TIMEOUT:
                failure = f'no result after {CHILD_TIMEOUT:.0f} s (exit codes {codes})'
            else:
                time.sleep(0.05)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        for p in procs:
            p.wait()
        for f in logs:
            f.close()
    print(f'{tag}: {time.time() - start:.1f} s')
    if failure is not None:
        tails = '\n'.join(open(f.name).read()[-3000:] for f in logs)
        raise AssertionError(f'{tag}: {failure}\n{tails}')
    return [torch.load(o, weights_only=False) for o in outs]


@pytest.mark.parametrize('kind', KINDS)
def test_two_ranks_over_gloo_equal_the_emulation(built_lib, tmp_path, kind):
    """needs no world invariance of the sampling launch: only that the collective moved the bytes, and that a gathered rollout
    trains through the ordered data-parallel mode to the bits of one process"""
    world = 2
    ranks = _run_world(kind, world, tmp_path)
    # the parent: a fresh agent (the children's seeds), the same shards one after another, trained at world 1
    ac = _agent(kind, AGENT_SEED[kind])
    rolls = [make_rollout(ac, (r, world), reward_fn) for r in range(world)]
    blocks, rows = [], []
    with torch.no_grad():
        for roll in rolls:
            roll.collect(T, seed=SEED)
            blocks.append(roll.pack().clone())
            rows.append(np.stack(roll._episode_stats, axis=1).reshape(-1, 2))
    data = rolls[0].unpack_gathered(torch.cat(blocks), T, on_device=True)
    assert data['obs'].world == world
    want_arrays = gathered_arrays(rolls[0])
    want = train(kind, ac, data)  # (ppo.train in one process takes a rollout gathered over any world)
    assert want['infos']['num_opt_steps'] == 3 and want['exp_avg'] is not None and bool(torch.isfinite(want['theta']).all())
    rows = np.concatenate(rows)
    for r, got in enumerate(ranks):
        for name, w in want_arrays.items():
            assert got['arrays'][name].dtype == w.dtype and torch.equal(got['arrays'][name].view(torch.uint8), w.view(torch.uint8)), (r, name)
        for k in ('theta', 'exp_avg', 'exp_avg_sq'):
            assert torch.equal(got[k], want[k]), (r, k)
        assert set(got['infos']) == set(want['infos'])
        for k in want['infos']:
            assert got['infos'][k] == want['infos'][k], (r, k, got['infos'][k], want['infos'][k])
        # global_statistics: the episodes of all ranks in rank order
        if len(rows):
            assert got['stats']['return_mean'] == np.mean(rows[:, 0]).item() and got['stats']['episode_length_std'] == np.std(rows[:, 1]).item()
        assert got['stats'] == ranks[0]['stats'] or all(np.isnan(v) for v in got['stats'].values())
