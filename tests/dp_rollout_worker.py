"""Subprocess body of tests/test_gpu_dp_rollout.py: one rank of a sharded device rollout over a real process group.
usage: python tests/dp_rollout_worker.py <covariant|internal> <rank> <world> <port> <out.pt>

Every rank builds the same agent (the seeds of tests/test_gpu_device_rollout.py), collects its share of the 5 environments,
calls `train_data()` -- the collective -- and trains 3 epochs in the ordered data-parallel mode.  gloo: all ranks share device 0."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import molgym_amd  # noqa: E402
from molgym_amd import ppo  # noqa: E402
from molgym_amd.rollout import DeviceRollout, _Views  # noqa: E402

NUM_ENVS, T, CAPACITY = 5, 4, 6
AGENT_SEED = {'covariant': 0, 'internal': 5}
GAMMA, LAM, MIN_REWARD, SEED = 0.99, 0.95, -0.25, 11  # tests/test_gpu_device_rollout.py


def make_rollout(ac, shard, reward_fn, num_envs=NUM_ENVS, capacity=CAPACITY):
    from tests.test_gpu_episodes import FORMULAS, MAX_SOLO, MIN_D
    return DeviceRollout(ac, FORMULAS, num_envs, capacity, gamma=GAMMA, lam=LAM, min_reward=MIN_REWARD, reward_fn=reward_fn,
                         min_atomic_distance=MIN_D, max_solo_distance=MAX_SOLO, shard=shard)


def gathered_arrays(roll, T=T):
    """{name: CPU tensor} of the used part of every array of the gathered store, and the gathered atom counts"""
    v = _Views(roll._gstore, roll._gtable, roll.num_envs * T)
    out = {name: getattr(v, name).cpu() for name in roll._gtable}
    out['natoms'] = torch.from_numpy(roll._gathered[1].copy())
    return out


def train(kind, ac, data):
    """3 epochs of the ordered data-parallel mode on `ac` itself; returns what the worlds must agree on"""
    molgym_amd.set_deterministic(True, covariant=(kind == 'covariant'), data_parallel=True)
    opt = torch.optim.Adam(ac.parameters(), lr=3e-4)
    np.random.seed(5)
    infos = ppo.train(ac, opt, data, mini_batch_size=6, clip_ratio=0.2, target_kl=1e9, vf_coef=0.5, entropy_coef=0.01, gradient_clip=0.5,
                      max_num_steps=3)
    torch.cuda.synchronize()
    st = opt.state.get(ac.theta, {})
    cpu = lambda t: None if t is None else t.detach().cpu()
    return {'theta': cpu(ac.theta), 'exp_avg': cpu(st.get('exp_avg')), 'exp_avg_sq': cpu(st.get('exp_avg_sq')),
            'infos': {k: v for k, v in infos.items() if k != 'time'}}


def main():
    kind, rank, world, port, out = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], sys.argv[5]
    from tests.test_gpu_device_rollout import reward_fn
    from tests.test_gpu_episodes import _agent
    torch.cuda.set_device(0)
    dist.init_process_group('gloo', init_method=f'tcp://127.0.0.1:{port}', rank=rank, world_size=world)
    ac = _agent(kind, AGENT_SEED[kind])
    roll = make_rollout(ac, (rank, world), reward_fn)
    with torch.no_grad():
        info = roll.collect(T, seed=SEED)
    stats = roll.global_statistics(info)
    data = roll.train_data(on_device=True)
    again = roll.train_data(on_device=True)  # cached: no second collective (a lone rank calling it would hang otherwise)
    assert data['obs'].world == world and len(data['obs']) == NUM_ENVS * T and again['adv'].data_ptr() == data['adv'].data_ptr()
    result = {'arrays': gathered_arrays(roll), 'stats': {k: v for k, v in stats.items() if k != 'time'}}
    result.update(train(kind, ac, data))
    torch.save(result, out)
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
