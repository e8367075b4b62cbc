"""Measurements for device rollouts under data parallelism (profiles/dp_device_rollout.md), on one GPU, SF6 (zs [0, 9, 16],
canvas 7), CovariantAC, zero reward, 140 environments x 10 steps, median of 7 repeats (fastest .. slowest).

  default   `shard=None`: from the first sampling launch to "`ppo.train` could start" (`collect` + `train_data()` +
            `prepare_rollout`), the timed region of tools/device_rollout_bench.py.  Uses nothing this feature added, so `--tree DIR`
            runs the same measurement on another checkout of the project (its parent commit); run each tree in several processes,
            alternating, for the spread between processes.
  exchange  world 8 emulated in one process: eight shards collect (untimed), their blocks are stacked as the collective stacks
            them; timed on one rank, alternating: `pack()` + `unpack_gathered()` (mg_traj_pack, mg_traj_unpack, mg_adv_normalize, the
            copy of the atom counts) against the same exchange written with sliced `copy_` calls (12 for the block, world x 12 for
            the gathered store, then the same normalise and copy).

usage: python tools/dp_rollout_bench.py default|exchange [--tree DIR] [num_envs] [steps] [repeats]"""
import os
import statistics
import sys
import time

argv = list(sys.argv[1:])
mode = argv.pop(0) if argv else 'default'
tree = '.'
if '--tree' in argv:
    at = argv.index('--tree')
    tree = argv[at + 1]
    del argv[at:at + 2]
sys.path.insert(0, os.path.abspath(tree))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import molgym_amd  # noqa: E402
from molgym_amd import _lib  # noqa: E402
from molgym_amd.agents.covariant import CovariantAC  # noqa: E402
from molgym_amd.rollout import DeviceRollout  # noqa: E402
from molgym_amd.spaces import ActionSpace, ObservationSpace  # noqa: E402
from molgym_amd.synthetic import CONFIGS, MODEL_DEFAULTS  # noqa: E402

E = int(argv[0]) if len(argv) > 0 else 140
steps = int(argv[1]) if len(argv) > 1 else 10
repeats = int(argv[2]) if len(argv) > 2 else 7
WORLD = 8
cfg = CONFIGS['cfg2']
zs, N = cfg['zs'], cfg['canvas_size']
formulas = [((16, 1), (9, 6))]  # SF6
GAMMA, LAM = 0.99, 0.97
torch.manual_seed(0)
ac = CovariantAC(ObservationSpace(N, zs), ActionSpace(zs), bag_scale=cfg['bag_scale'], beta=cfg['beta'], device=torch.device('cuda'),
                 **MODEL_DEFAULTS)
dev = ac.theta.device


def fmt(v):
    return f'{statistics.median(v) * 1e3:.3f} ({min(v) * 1e3:.3f} .. {max(v) * 1e3:.3f})'


def default_mode():
    roll = DeviceRollout(ac, formulas, E, steps, gamma=GAMMA, lam=LAM, min_reward=0.0)

    def run(seed):
        roll.reset()
        torch.manual_seed(seed)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        roll.collect(steps)
        ac.prepare_rollout(roll.train_data())
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    with torch.no_grad():
        run(0)
        times = [run(100 + rep) for rep in range(repeats)]
    print(f'default | tree {os.path.abspath(tree)} (molgym_amd from {os.path.dirname(molgym_amd.__file__)}, ABI {_lib.ABI_VERSION}) | '
          f'{E} x {steps} | collect + train_data + prepare_rollout: {fmt(times)} ms')


def exchange_mode():
    from molgym_amd.rollout import _Views, exchange_layout, shard_bounds, store_layout
    rolls = [DeviceRollout(ac, formulas, E, steps, gamma=GAMMA, lam=LAM, min_reward=0.0, shard=(r, WORLD)) for r in range(WORLD)]
    with torch.no_grad():
        for roll in rolls:
            roll.collect(steps, seed=3)
    stacked = torch.cat([roll.pack().clone() for roll in rolls])
    me = rolls[3]
    sections, block_bytes = exchange_layout(E, WORLD, steps, N, len(zs), 6)
    gtable, gbytes = store_layout(E, steps, N, len(zs), 6)
    size = lambda dtype: 8 if dtype == torch.float64 else 4
    block2 = torch.zeros(block_bytes, dtype=torch.uint8, device=dev)
    gstore2 = torch.zeros(gbytes, dtype=torch.uint8, device=dev)
    natoms2 = torch.zeros(E * steps, dtype=torch.int32, device=dev)
    p = lambda t: __import__('ctypes').c_void_p(t.data_ptr())

    def kernels():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        me.pack()
        me.unpack_gathered(stacked, steps, on_device=True)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def copies():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        v = me._views()
        S = me.E * steps
        natoms = torch.from_numpy(np.ascontiguousarray(me._natoms_hist.reshape(-1), dtype=np.int32)).to(dev)
        for name, (off, dtype, k) in sections.items():  # 12 copies: the block
            src = natoms if name == 'natoms' else getattr(v, name)
            block2[off:off + S * k * size(dtype)].copy_(src.view(torch.uint8))
        for r in range(WORLD):  # world x 12 copies: the gathered store
            lo, hi = shard_bounds(E, r, WORLD)
            for name, (off, dtype, k) in sections.items():
                per = steps * k * size(dtype)
                src = stacked[r * block_bytes + off:r * block_bytes + off + (hi - lo) * per]
                if name == 'natoms':
                    natoms2.view(torch.uint8)[lo * per:hi * per].copy_(src)
                else:
                    goff = gtable[name][0]
                    gstore2[goff + lo * per:goff + hi * per].copy_(src)
        g = _Views(gstore2, gtable, E * steps)
        with ac._guard():
            _lib.check(_lib.lib().mg_adv_normalize(E * steps, p(g.adv), None, ac._s()))
        natoms2.cpu().numpy()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    kernels(), copies()
    same = torch.equal(gstore2, me._gstore) and torch.equal(block2, me._block)
    a, b = [], []
    for rep in range(repeats):
        a.append(kernels())
        b.append(copies())
    print(f'exchange | world {WORLD} emulated, {E} x {steps}, block {block_bytes} bytes, gathered store {gbytes} bytes | '
          f'the two routes give the same bytes: {same}')
    print(f'| pack + unpack_gathered (mg_traj_pack, mg_traj_unpack, mg_adv_normalize, natoms copy) | {fmt(a)} ms |')
    print(f'| the same with {12 + WORLD * 12} sliced copy_ calls | {fmt(b)} ms |')


if mode == 'default':
    default_mode()
elif mode == 'exchange':
    exchange_mode()
else:
    sys.exit(f'{mode}: default or exchange')
