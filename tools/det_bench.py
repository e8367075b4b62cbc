"""Cost of deterministic mode on the GPU box: both agents, mode off / on, (1) the PPO mini-batch step at the SF6 mini-batch size
(140 samples, canvas 7) and (2) molgym_amd.ppo.train end to end (tools/train_bench.py's loop).  Modes alternate inside one process,
three rounds, so each figure comes with its own spread; device work is closed by a synchronise before the clock is read.
usage: python tools/det_bench.py [steps per window = 200] [rollout samples = 1400] [epochs = 5]"""
import sys
import time

import numpy as np
import torch

sys.path.insert(0, '.')
import molgym_amd  # noqa: E402
from molgym_amd import ppo  # noqa: E402
from molgym_amd.agents.covariant import CovariantAC  # noqa: E402
from molgym_amd.agents.internal import SchNetAC  # noqa: E402
from molgym_amd.spaces import ActionSpace, ObservationSpace  # noqa: E402
from molgym_amd.synthetic import CONFIGS, MODEL_DEFAULTS, make_batch, make_batch_internal  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
n = int(sys.argv[2]) if len(sys.argv) > 2 else 1400
epochs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
HP = (0.2, 0.5, 0.01)
cfg = CONFIGS['cfg2']
zs, N, mb = cfg['zs'], cfg['canvas_size'], cfg['batch']


def agent(kind):
    torch.manual_seed(0)
    if kind == 'internal':
        return SchNetAC(ObservationSpace(N, zs), ActionSpace(zs), (0.8, 1.8), 128, device='cuda:0')
    return CovariantAC(ObservationSpace(N, zs), ActionSpace(zs), bag_scale=cfg['bag_scale'], beta=cfg['beta'], device='cuda:0',
                       **MODEL_DEFAULTS)


def set_mode(kind, on):
    molgym_amd.set_deterministic(on, covariant=(on and kind == 'covariant'))


for kind in ('covariant', 'internal'):
    make = make_batch_internal if kind == 'internal' else make_batch
    ac = agent(kind)
    d = make(mb, N, zs, seed=0)
    batch = ac.prepare_batch(d['obs'], d['act'], d['logp'], d['adv'], d['ret'])
    ms = {False: [], True: []}
    for rnd in range(3):
        for on in (False, True):
            set_mode(kind, on)
            ac.theta.grad = torch.zeros_like(ac.theta)
            for _ in range(10):
                ac.ppo_minibatch(batch, *HP)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                ac.ppo_minibatch(batch, *HP)
            torch.cuda.synchronize()
            ms[on].append((time.perf_counter() - t0) / steps * 1e3)
    for on in (False, True):
        print(f'{kind} ppo_minibatch B={mb} canvas {N}, deterministic={on}: ms per step {["%.4f" % x for x in ms[on]]} '
              f'(median {np.median(ms[on]):.4f})')
    print(f'{kind} ppo_minibatch: mode on / off = {np.median(ms[True]) / np.median(ms[False]):.2f}x')
    d = make(n, N, zs, seed=0)
    data = {k: d[k] for k in ('obs', 'act', 'logp', 'adv', 'ret')}
    tr = {False: [], True: []}
    for rnd in range(3):
        for on in (False, True):
            set_mode(kind, on)
            ac2 = agent(kind)
            opt = torch.optim.Adam(ac2.parameters(), lr=1e-5)
            for timed in (False, True):  # the first call warms every shape of the loop
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                info = ppo.train(ac2, opt, data, mini_batch_size=mb, clip_ratio=0.2, target_kl=1e9, vf_coef=0.5, entropy_coef=0.01,
                                 gradient_clip=0.5, max_num_steps=epochs)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
            tr[on].append(dt / max(info['num_opt_steps'], 1) / (n / mb) * 1e3)
    for on in (False, True):
        print(f'{kind} ppo.train rollout {n}, mini-batch {mb}, {epochs} epochs, deterministic={on}: ms per mini-batch '
              f'{["%.4f" % x for x in tr[on]]} (median {np.median(tr[on]):.4f})')
    print(f'{kind} ppo.train: mode on / off = {np.median(tr[True]) / np.median(tr[False]):.2f}x')
    molgym_amd.set_deterministic(False)
