"""Subprocess body of tests/test_gpu_dp_ordered.py: one rank of `ppo.train` in the ordered data-parallel mode.
usage: python tests/dp_ordered_worker.py <schnet|covariant> <gloo|nccl> <rank> <world> <port> <out.pt>

Every rank builds the same agent and the same 70-sample rollout from the same seeds (the shapes of
tests/test_gpu_internal_deterministic.py::test_train_twice_gives_the_same_bits: canvas 7, ZS = [0, 9, 16], width 64, mini-batches
of 20, recorded log-probs 0.05 above the agent's own), turns the three switches on and trains 3 epochs under both target_kl values
of that test.  gloo: all ranks share device 0; nccl: rank r takes device r."""
import copy
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import molgym_amd  # noqa: E402
from molgym_amd import ppo  # noqa: E402
from molgym_amd.spaces import ActionSpace, ObservationSpace  # noqa: E402
from molgym_amd.synthetic import CONFIGS, MODEL_DEFAULTS, make_batch, make_batch_internal  # noqa: E402

ZS = [0, 9, 16]
CANVAS, WIDTH = 7, 64


def build_agent(kind, device, seed=12):
    torch.manual_seed(seed)
    if kind == 'schnet':
        from molgym_amd.agents.internal import SchNetAC
        ac = SchNetAC(ObservationSpace(CANVAS, ZS), ActionSpace(ZS), (0.8, 1.8), WIDTH, device=device)
    else:
        from molgym_amd.agents.covariant import CovariantAC
        cfg = CONFIGS['cfg2']
        assert cfg['zs'] == ZS and cfg['canvas_size'] == CANVAS
        ac = CovariantAC(ObservationSpace(CANVAS, ZS), ActionSpace(ZS), bag_scale=cfg['bag_scale'], beta=cfg['beta'], device=device,
                         **dict(MODEL_DEFAULTS, network_width=WIDTH))
    with torch.no_grad():  # non-trivial biases, so that every gradient path carries something
        g = torch.Generator().manual_seed(seed + 1)
        for name, (off, shape) in ac.slot_table.items():
            n = int(np.prod(shape))
            if name.endswith('bias'):
                ac.theta[off:off + n] = (0.1 * torch.randn(n, generator=g)).to(ac.theta)
    return ac


def build_data(kind, ac, n=70, seed=21):
    data = (make_batch_internal if kind == 'schnet' else make_batch)(n, CANVAS, ZS, seed=seed)
    with torch.no_grad():
        data['logp'] = ac.step(data['obs'], data['act'])['logp'].double().cpu().numpy() + 0.05
    return data


def main():
    kind, backend, rank, world, port, out = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5], sys.argv[6]
    index = rank if backend == 'nccl' and torch.cuda.device_count() >= world else 0
    torch.cuda.set_device(index)
    dev = torch.device('cuda', index)
    kw = {'device_id': dev} if backend == 'nccl' else {}
    dist.init_process_group(backend, init_method=f'tcp://127.0.0.1:{port}', rank=rank, world_size=world, **kw)
    base = build_agent(kind, f'cuda:{index}')
    data = build_data(kind, base)
    molgym_amd.set_deterministic(True, covariant=(kind == 'covariant'), data_parallel=True)
    runs = []
    for target_kl in (1e9, 0.01):
        ac = copy.deepcopy(base)
        opt = torch.optim.Adam(ac.parameters(), lr=3e-4)
        np.random.seed(5)
        infos = ppo.train(ac, opt, data, mini_batch_size=20, clip_ratio=0.2, target_kl=target_kl, vf_coef=0.5, entropy_coef=0.01,
                          gradient_clip=0.5, max_num_steps=3)
        torch.cuda.synchronize()
        st = opt.state.get(ac.theta, {})
        cpu = lambda t: None if t is None else t.detach().cpu()
        runs.append({'target_kl': target_kl, 'theta': cpu(ac.theta), 'exp_avg': cpu(st.get('exp_avg')),
                     'exp_avg_sq': cpu(st.get('exp_avg_sq')), 'infos': {k: v for k, v in infos.items() if k != 'time'},
                     'moved': not torch.equal(ac.theta.detach(), base.theta.detach())})
    torch.save(runs, out)
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
