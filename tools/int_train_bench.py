"""Measurement (GPU box): one `ppo.train` call for SchNetAC on the rollout of a device collect, handed over in three forms --
  host     `DeviceRollout.data()`: `IntRollout`, every mini-batch assembled on the host and uploaded,
  gather   the same host data with `gather_on_device`: parked once, every mini-batch one `mg_int_gather_batch`,
  carried  `train_data(on_device=True)`: the store's own arrays, nothing uploaded, the same gather --
alternating call by call in one process (`prepare_rollout` is inside the timed call, the copy back of `data()` is not); median
of the repeats with the fastest and the slowest.  SF6 on canvas 7, or a 28-atom bag (S4 F24) on a wider canvas.  A collect of an
untrained policy holds few atoms per canvas; `synthetic` times `synthetic.make_batch_internal` instead (atom counts uniform in
0 .. canvas, no store, so no carried form).
usage: python tools/int_train_bench.py [canvas] [num_envs] [steps] [mini batch] [epochs] [repeats] [synthetic]  (prints markdown)"""
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, '.')
from molgym_amd import ppo  # noqa: E402
from molgym_amd.agents.internal import SchNetAC  # noqa: E402
from molgym_amd.rollout import DeviceRollout  # noqa: E402
from molgym_amd.spaces import ActionSpace, ObservationSpace  # noqa: E402

arg = lambda i, default: int(sys.argv[i]) if len(sys.argv) > i else default
N, E, steps, mb, epochs, repeats = arg(1, 7), arg(2, 140), arg(3, 10), arg(4, 140), arg(5, 5), arg(6, 7)
zs = [0, 9, 16]
formulas = [((16, 1), (9, 6))] if N <= 7 else [((16, 4), (9, 24))]
torch.manual_seed(0)
ac = SchNetAC(ObservationSpace(N, zs), ActionSpace(zs), (0.8, 1.8), 128, device='cuda:0')
synthetic = len(sys.argv) > 7 and sys.argv[7] == 'synthetic'
if synthetic:
    from molgym_amd.synthetic import make_batch_internal  # noqa: E402
    d = make_batch_internal(E * steps, N, zs, seed=0)
    host_data, carried = {k: d[k] for k in ('obs', 'act', 'logp', 'adv', 'ret')}, None
    natoms = np.array([sum(1 for label, _ in canvas if label) for canvas, _ in d['obs']])
else:
    roll = DeviceRollout(ac, formulas, E, steps, gamma=0.99, lam=0.97, min_reward=0.0)
    with torch.no_grad():
        roll.collect(steps, seed=1)
    natoms = roll._natoms_hist.reshape(-1)
    host_data, carried = roll.data(), roll.train_data(on_device=True)
opt = torch.optim.Adam(ac.parameters(), lr=1e-5)


def train(form):
    ac.gather_on_device = form == 'gather'
    data = carried if form == 'carried' else host_data
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    info = ppo.train(ac, opt, data, mini_batch_size=mb, clip_ratio=0.2, target_kl=1e9, vf_coef=0.5, entropy_coef=0.01,
                     gradient_clip=0.5, max_num_steps=epochs)
    torch.cuda.synchronize()
    assert info['num_opt_steps'] == epochs
    return time.perf_counter() - t0


forms = ('host', 'gather') if synthetic else ('host', 'gather', 'carried')
for f in forms:  # warm-up: workspaces, graphs
    train(f)
rows = {f: [] for f in forms}
for rep in range(repeats):
    for f in forms:
        rows[f].append(train(f))
S = E * steps
print(f'SchNetAC, width 128, canvas {N}, {"synthetic " if synthetic else ""}rollout of {S} samples ({E} environments x {steps} steps, {natoms.mean():.1f} atoms per canvas on '
      f'average, at most {natoms.max()}), mini-batches of {mb}, {epochs} epochs; median of {repeats} alternating calls (fastest .. slowest)\n')
print('| form of the rollout | one `ppo.train` call, ms | samples/s | against host |')
print('|---|---|---|---|')
base = statistics.median(rows['host'])
for f in forms:
    m = statistics.median(rows[f])
    print(f'| {f} | {m * 1e3:.2f} ({min(rows[f]) * 1e3:.2f} .. {max(rows[f]) * 1e3:.2f}) | {S * epochs / m:.0f} | {base / m:.3f} x |')
