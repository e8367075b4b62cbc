"""numpy statement of `mg_traj_pack` / `mg_traj_unpack` (include/molgym_hip.h) on `rollout.exchange_layout`: stores and blocks
are uint8 arrays, every copy is a slice assignment of bytes."""
import numpy as np
import torch

from molgym_amd import rollout


def _size(dtype) -> int:
    return 8 if dtype == torch.float64 else 4


def random_store(rng, num_envs, capacity, N, Z, cols):
    """a store of `num_envs * capacity` samples filled with random bytes (padding between the arrays included)"""
    nbytes = rollout.store_layout(num_envs, capacity, N, Z, cols)[1]
    return rng.integers(0, 256, size=nbytes, dtype=np.uint8)


def pack(store, natoms, num_envs, world, rank, T, capacity, N, Z, cols, block=None):
    """the send block of `rank`: `store` is its own store (`hi - lo` environments, `capacity` steps), `natoms` its int32 atom
    counts ((hi - lo) * T,); a block that is passed in is written in place (what lies beyond the sections' used parts stays)"""
    lo, hi = rollout.shard_bounds(num_envs, rank, world)
    table = rollout.store_layout(hi - lo, capacity, N, Z, cols)[0]
    sections, block_bytes = rollout.exchange_layout(num_envs, world, T, N, Z, cols)
    if block is None:
        block = np.zeros(block_bytes, dtype=np.uint8)
    assert block.shape == (block_bytes, ) and block.dtype == np.uint8
    S = (hi - lo) * T
    for name, (off, dtype, k) in sections.items():
        n = S * k * _size(dtype)
        if name == 'natoms':
            block[off:off + n] = np.ascontiguousarray(natoms, dtype=np.int32).reshape(-1).view(np.uint8)
        else:
            src = table[name][0]
            block[off:off + n] = store[src:src + n]
    return block


def unpack(blocks, num_envs, world, T, capacity, N, Z, cols, store=None, natoms=None):
    """(gathered store, gathered natoms (num_envs * T,) int32) from `blocks` [world][block_bytes]; arrays passed in are written
    in place"""
    table, nbytes = rollout.store_layout(num_envs, capacity, N, Z, cols)
    sections, block_bytes = rollout.exchange_layout(num_envs, world, T, N, Z, cols)
    blocks = np.asarray(blocks, dtype=np.uint8).reshape(world, block_bytes)
    if store is None:
        store = np.zeros(nbytes, dtype=np.uint8)
    if natoms is None:
        natoms = np.zeros(num_envs * T, dtype=np.int32)
    raw = natoms.view(np.uint8)
    for r in range(world):
        lo, hi = rollout.shard_bounds(num_envs, r, world)
        for name, (off, dtype, k) in sections.items():
            per = T * k * _size(dtype)  # bytes per environment
            src = blocks[r, off:off + (hi - lo) * per]
            if name == 'natoms':
                raw[lo * per:hi * per] = src
            else:
                dst = table[name][0]
                store[dst + lo * per:dst + hi * per] = src
    return store, natoms
