"""The host side of device rollouts under data parallelism (molgym_amd/rollout.py): the split, the block layout, the numpy mirror
of the two exchange kernels (tests/exchange_ref.py), `ppo.train`'s acceptance of a gathered rollout and the all-gather helper
over gloo.  No GPU."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from molgym_amd import ppo, rollout
from molgym_amd.observations import CarriedRollout
from tests import exchange_ref as X


def test_shard_bounds_partition_the_environments():
    for num_envs in (5, 7, 70, 140):
        for world in range(1, 6):
            bounds = [rollout.shard_bounds(num_envs, r, world) for r in range(world)]
            assert bounds[0][0] == 0 and bounds[-1][1] == num_envs
            assert all(a[1] == b[0] for a, b in zip(bounds, bounds[1:]))
            sizes = [hi - lo for lo, hi in bounds]
            assert min(sizes) >= 1 and max(sizes) - min(sizes) <= 1 and max(sizes) == -(-num_envs // world)
            # the split of ppo._shard_global_config
            assert bounds == [((r * num_envs) // world, ((r + 1) * num_envs) // world) for r in range(world)]
    assert [rollout.shard_bounds(5, r, 2) for r in range(2)] == [(0, 2), (2, 5)]
    assert [rollout.shard_bounds(5, r, 3) for r in range(3)] == [(0, 1), (1, 3), (3, 5)]
    with pytest.raises(ValueError, match='world'):
        rollout.shard_bounds(5, 0, 0)
    for rank in (-1, 3):
        with pytest.raises(ValueError, match='rank'):
            rollout.shard_bounds(5, rank, 3)
    with pytest.raises(ValueError, match='environments'):
        rollout.shard_bounds(2, 0, 3)


@pytest.mark.parametrize('num_envs,world,T,N,Z,cols', [(5, 3, 4, 6, 4, 6), (5, 2, 4, 6, 4, 7), (3, 2, 1, 255, 16, 7), (70, 3, 3, 7, 3, 6),
                                                        (140, 8, 10, 7, 3, 6)])
def test_exchange_layout(num_envs, world, T, N, Z, cols):
    sections, block_bytes = rollout.exchange_layout(num_envs, world, T, N, Z, cols)
    names = [name for name, _, _ in rollout._FIELDS]
    assert list(sections) == names + ['natoms'] and sections['natoms'][1:] == (torch.int32, 1)
    share = -(-num_envs // world) * T
    table = rollout.store_layout(num_envs, T, N, Z, cols)[0]
    end = 0
    for name, (off, dtype, k) in sections.items():
        assert off % 256 == 0 and off >= end, name
        if name != 'natoms':
            assert (dtype, k) == table[name][1:], name
        end = off + share * k * (8 if dtype == torch.float64 else 4)
    assert end <= block_bytes < end + 256 and block_bytes % 256 == 0
    # the byte count does not depend on the rank: the layout has no rank argument, and every share fits its section
    assert all(rollout.shard_bounds(num_envs, r, world)[1] - rollout.shard_bounds(num_envs, r, world)[0] <= share // T for r in range(world))
    with pytest.raises(ValueError):
        rollout.exchange_layout(2, 3, T, N, Z, cols)


@pytest.mark.parametrize('num_envs,world', [(5, 3), (70, 3)])  # shares (1, 2, 2) and (23, 23, 24)
def test_numpy_mirror_round_trip(num_envs, world):
    T, capacity, N, Z, cols = 4, 6, 6, 4, 7
    rng = np.random.default_rng(num_envs)
    shares = [rollout.shard_bounds(num_envs, r, world) for r in range(world)]
    assert [hi - lo for lo, hi in shares] == ([1, 2, 2] if num_envs == 5 else [23, 23, 24])
    stores = [X.random_store(rng, hi - lo, capacity, N, Z, cols) for lo, hi in shares]
    natoms = [rng.integers(0, N, size=(hi - lo) * T).astype(np.int32) for lo, hi in shares]
    block_bytes = rollout.exchange_layout(num_envs, world, T, N, Z, cols)[1]
    blocks = np.stack([X.pack(stores[r], natoms[r], num_envs, world, r, T, capacity, N, Z, cols) for r in range(world)])
    assert blocks.shape == (world, block_bytes)
    gathered, gnatoms = X.unpack(blocks, num_envs, world, T, capacity, N, Z, cols)
    assert np.array_equal(gnatoms, np.concatenate(natoms))
    gtable = rollout.store_layout(num_envs, capacity, N, Z, cols)[0]
    for name, (goff, dtype, k) in gtable.items():
        per = T * k * (8 if dtype == torch.float64 else 4)
        for r, (lo, hi) in enumerate(shares):
            loff = rollout.store_layout(hi - lo, capacity, N, Z, cols)[0][name][0]
            assert np.array_equal(gathered[goff + lo * per:goff + hi * per], stores[r][loff:loff + (hi - lo) * per]), (name, r)
        # what lies behind the used part of the gathered array was not written
        assert not gathered[goff + num_envs * per:goff + num_envs * capacity * k * (8 if dtype == torch.float64 else 4)].any(), name
    # a short share leaves the tail of its sections as the block held it
    poisoned = np.full(block_bytes, 0xFF, dtype=np.uint8)
    X.pack(stores[0], natoms[0], num_envs, world, 0, T, capacity, N, Z, cols, block=poisoned)
    sections = rollout.exchange_layout(num_envs, world, T, N, Z, cols)[0]
    lo, hi = shares[0]
    written = np.zeros(block_bytes, dtype=bool)
    for name, (off, dtype, k) in sections.items():
        written[off:off + (hi - lo) * T * k * (8 if dtype == torch.float64 else 4)] = True
    assert (poisoned[~written] == 0xFF).all() and (~written).sum() > 0 and np.array_equal(poisoned[written], blocks[0][written])


def test_train_takes_a_rollout_gathered_over_its_world(monkeypatch):
    monkeypatch.setattr(ppo, '_dist', lambda: (object(), 0, 2))
    args = (4, 0.2, 0.01, 0.5, 0.01, 0.5, 2)
    plain = CarriedRollout(12, object())
    assert plain.world == 1
    with pytest.raises(RuntimeError, match='world size 2'):
        ppo.train(None, None, dict(obs=plain, act=None, ret=None, adv=None, logp=None), *args)
    three = CarriedRollout(12, object())
    three.world = 3
    with pytest.raises(RuntimeError, match='world size 2'):
        ppo.train(None, None, dict(obs=three, act=None, ret=None, adv=None, logp=None), *args)
    two = CarriedRollout(12, object())
    two.world = 2
    with pytest.raises(Exception) as err:  # past the check: the stand-in agent (None) fails later, with another error
        ppo.train(None, None, dict(obs=two, act=None, ret=None, adv=None, logp=None), *args)
    assert 'world size' not in str(err.value)


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _gather_worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    torch.set_num_threads(1)
    calls = []
    for name in ('all_gather', 'all_gather_into_tensor', 'all_reduce', 'broadcast', 'all_gather_object', 'gather', 'all_to_all'):
        def counted(*a, _f=getattr(dist, name), _n=name, **kw):
            calls.append(_n)
            return _f(*a, **kw)
        setattr(dist, name, counted)
    block = torch.full((1024, ), 17 + rank, dtype=torch.uint8)
    block[:8] = torch.arange(8, dtype=torch.uint8) * (rank + 1)
    got = rollout.all_gather_blocks(block)
    torch.save({'got': got, 'calls': calls}, f'{out}.r{rank}.pt')
    dist.destroy_process_group()


def test_all_gather_blocks_over_gloo_is_one_collective(tmp_path):
    out = str(tmp_path / 'gather')
    mp.spawn(_gather_worker, args=(2, _free_port(), out), nprocs=2, join=True)
    want = []
    for rank in range(2):
        block = torch.full((1024, ), 17 + rank, dtype=torch.uint8)
        block[:8] = torch.arange(8, dtype=torch.uint8) * (rank + 1)
        want.append(block)
    want = torch.cat(want)
    for rank in range(2):
        res = torch.load(f'{out}.r{rank}.pt', weights_only=False)
        assert res['calls'] == ['all_gather'], res['calls']
        assert res['got'].dtype == torch.uint8 and torch.equal(res['got'], want), rank
    # without a process group the block is its own gathering
    alone = torch.arange(16, dtype=torch.uint8)
    assert torch.equal(rollout.all_gather_blocks(alone), alone)
