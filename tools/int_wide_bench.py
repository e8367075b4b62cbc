"""SchNetAC PPO mini-batch (forward + float64 loss + backward, one call) on wide canvases: bench.py's internal leg is fixed at
canvas 7.  Prints one JSON line: ms per step over --steps after --warmup.

usage: python tools/int_wide_bench.py [--canvas 128] [--batch 140] [--steps 50] [--warmup 10]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--canvas', type=int, default=128)
    p.add_argument('--batch', type=int, default=140)
    p.add_argument('--steps', type=int, default=50)
    p.add_argument('--warmup', type=int, default=10)
    args = p.parse_args()
    import torch
    from molgym_amd.agents.internal import SchNetAC
    from molgym_amd.spaces import ActionSpace, ObservationSpace
    from molgym_amd.synthetic import make_batch_internal
    zs, N, B = [0, 1, 6, 7, 8], args.canvas, args.batch
    torch.manual_seed(0)
    ac = SchNetAC(ObservationSpace(N, zs), ActionSpace(zs), (0.8, 1.8), 128, device='cuda:0')
    data = make_batch_internal(B, N, zs, seed=0)
    batch = ac.prepare_batch(data['obs'], data['act'], data['logp'], data['adv'], data['ret'])
    ac.theta.grad = torch.zeros_like(ac.theta)
    for _ in range(args.warmup):
        ac.ppo_minibatch(batch, 0.2, 0.5, 0.01)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        stats = ac.ppo_minibatch(batch, 0.2, 0.5, 0.01)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    if not torch.isfinite(stats).all():
        raise SystemExit('non-finite loss statistics')
    natoms = [sum(1 for it in o[0] if it[0] != 0) for o in data['obs']]
    print(json.dumps({'agent': 'internal', 'canvas_size': N, 'mini_batch': B, 'atoms': int(sum(natoms)),
                      'ms_per_step': dt * 1e3, 'samples_per_s': B / dt, 'steps': args.steps, 'warmup': args.warmup}))


if __name__ == '__main__':
    main()
