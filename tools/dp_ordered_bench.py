"""Cost of the ordered data-parallel mode at world 1 (GPU box): wall-clock time of one molgym_amd.ppo.train call, SchNetAC on
BASELINE configs[0] (canvas 7, width 128), a 1400-sample rollout in mini-batches of 140, deterministic mode on, with the third
switch (set_deterministic(..., data_parallel=True)) off and on -- and the same call in a checkout of the parent commit (`--parent
DIR`, with `__graft_entry__.build()` run in it: its own library AND its host-side observation parser, or prepare_rollout is
timed on the numpy parser there), started from here as a child process.  The modes alternate call by call inside one process; every figure is
the median of `calls` train calls after warm-up, device work closed by a synchronise before the clock is read.

usage: python tools/dp_ordered_bench.py [--parent DIR] [--calls 20] [--epochs 5] [--rounds 3] [--out profiles/r12_dp_ordered.txt]
       python tools/dp_ordered_bench.py --measure [--calls 20] [--epochs 5]     (one JSON line: what --parent runs in DIR)"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

N, MB, WIDTH, CANVAS, ZS = 1400, 140, 128, 7, [0, 9, 16]


def measure(calls, epochs):
    import torch
    sys.path.insert(0, os.getcwd())
    import molgym_amd
    from molgym_amd import ppo
    from molgym_amd.agents.internal import SchNetAC
    from molgym_amd.spaces import ActionSpace, ObservationSpace
    from molgym_amd.synthetic import make_batch_internal
    has_switch = hasattr(molgym_amd, 'is_deterministic_data_parallel')  # (the parent commit has no third switch)
    modes = [False, True] if has_switch else [False]
    d = make_batch_internal(N, CANVAS, ZS, seed=0)
    data = {k: d[k] for k in ('obs', 'act', 'logp', 'adv', 'ret')}
    agents = {}
    for on in modes:
        torch.manual_seed(0)
        ac = SchNetAC(ObservationSpace(CANVAS, ZS), ActionSpace(ZS), (0.8, 1.8), WIDTH, device='cuda:0')
        agents[on] = (ac, torch.optim.Adam(ac.parameters(), lr=1e-5))
    ms = {on: [] for on in modes}
    for call in range(3 + calls):  # three warm-up calls per mode
        for on in modes:
            if on:
                molgym_amd.set_deterministic(True, data_parallel=True)
            else:
                molgym_amd.set_deterministic(True)
            ac, opt = agents[on]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            info = ppo.train(ac, opt, data, mini_batch_size=MB, clip_ratio=0.2, target_kl=1e9, vf_coef=0.5, entropy_coef=0.01,
                             gradient_clip=0.5, max_num_steps=epochs)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            assert info['num_opt_steps'] == epochs
            if call >= 3:
                ms[on].append(dt)
    molgym_amd.set_deterministic(False)
    out = {'switch_off_ms': float(np.median(ms[False])), 'switch_off_min_max': [min(ms[False]), max(ms[False])]}
    if has_switch:
        out.update(switch_on_ms=float(np.median(ms[True])), switch_on_min_max=[min(ms[True]), max(ms[True])])
    print('RESULT ' + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--measure', action='store_true')
    ap.add_argument('--parent', default=None)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--epochs', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=os.path.join('profiles', 'r12_dp_ordered.txt'))
    args = ap.parse_args()
    if args.measure:
        return measure(args.calls, args.epochs)

    def child(cwd):
        res = subprocess.run([sys.executable, os.path.abspath(__file__), '--measure', '--calls', str(args.calls), '--epochs',
                              str(args.epochs)], cwd=cwd, capture_output=True, text=True, timeout=600)
        if res.returncode != 0:
            raise RuntimeError(res.stdout[-2000:] + res.stderr[-4000:])
        return json.loads([ln for ln in res.stdout.splitlines() if ln.startswith('RESULT ')][-1][7:])

    # this tree and the parent's alternate, process by process: a difference between the two must show in every round
    here, parent = [], []
    for _ in range(args.rounds):
        here.append(child(os.getcwd()))
        if args.parent:
            parent.append(child(args.parent))
    med = lambda runs, key: float(np.median([r[key] for r in runs]))
    each = lambda runs, key: ', '.join(f'{r[key]:.3f}' for r in runs)
    lines = ['Ordered data-parallel mode (molgym_amd.set_deterministic(True, data_parallel=True)) at world 1: cost of one ppo.train call.',
             f'SchNetAC, BASELINE configs[0] (canvas {CANVAS}, width {WIDTH}), rollout {N}, mini-batches of {MB}, {args.epochs} epochs per call;',
             f'deterministic mode on throughout; median of {args.calls} calls after 3 warm-up calls, the two settings of the switch',
             f'alternating call by call inside one process; {args.rounds} processes per tree, this tree and the parent commit\'s alternating.',
             '(tools/dp_ordered_bench.py; ms per train call: median over the processes, then each process)', '']
    off, on = med(here, 'switch_off_ms'), med(here, 'switch_on_ms')
    if parent:
        lines.append(f'parent commit, deterministic ppo.train:         {med(parent, "switch_off_ms"):8.3f}   ({each(parent, "switch_off_ms")})')
    lines.append(f'this commit, deterministic, third switch off:   {off:8.3f}   ({each(here, "switch_off_ms")})')
    lines.append(f'this commit, deterministic, third switch on:    {on:8.3f}   ({each(here, "switch_on_ms")})')
    lines.append(f'switch on / switch off (this commit):           {on / off:8.3f}')
    if parent:
        lines.append(f'switch on / parent commit:                      {on / med(parent, "switch_off_ms"):8.3f}')
        lines.append(f'switch off / parent commit:                     {off / med(parent, "switch_off_ms"):8.3f}')
    text = '\n'.join(lines) + '\n'
    print(text)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
