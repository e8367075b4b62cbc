"""Measurement (GPU box): `DeviceRollout.collect` with a placed atom paid
  (a) nothing           `reward_fn=None`
  (b) on the host       `reward_fn=PairReward(...).host`: per-row Python lists, the reward loop, two uploads per step
  (c) on the device     `reward=PairReward(...)`: `mg_traj_pair_reward` + `mg_episode_cut` behind `mg_traj_status`, one 12-byte-per-
                        environment copy per step
in the configuration of tools/device_rollout_bench.py -- SF6 (zs [0, 9, 16]), canvas 7, 140 environments x 10 steps -- for
CovariantAC and SchNetAC, and for CovariantAC on a canvas of 40 that starts from a 24-atom structure (every reward sums 24 pairs
or more).  The three settings alternate in one process; median of the repeats with the fastest and the slowest.  Made-up
Lennard-Jones parameters; (b) and (c) pay the same bits, so they walk the same trajectories ((a) pays 0.0 and cuts nothing: its
episodes differ).
usage: python tools/pair_reward_bench.py [--only a] [--json] [num_envs] [steps] [repeats] [out.md]   (default out: profiles/pair_reward.md)"""
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, '.')
from molgym_amd.rollout import DeviceRollout  # noqa: E402
from molgym_amd.agents.covariant import CovariantAC  # noqa: E402
from molgym_amd.agents.internal import SchNetAC  # noqa: E402
from molgym_amd.spaces import ActionSpace, ObservationSpace  # noqa: E402
from molgym_amd.synthetic import CONFIGS, MODEL_DEFAULTS  # noqa: E402

argv = list(sys.argv[1:])
only_a, as_json = '--only' in argv, '--json' in argv
if only_a:
    del argv[argv.index('--only'):argv.index('--only') + 2]
if as_json:
    argv.remove('--json')
E = int(argv[0]) if len(argv) > 0 else 140
steps = int(argv[1]) if len(argv) > 1 else 10
repeats = int(argv[2]) if len(argv) > 2 else 7
out_path = argv[3] if len(argv) > 3 else 'profiles/pair_reward.md'
cfg = CONFIGS['cfg2']
zs = cfg['zs']
GAMMA, LAM, MIN_REWARD = 0.99, 0.97, -0.6
EPS, SIGMA = (0.0, 0.09, 0.12), (0.0, 1.40, 1.55)


def agent_of(kind, N):
    torch.manual_seed(0)
    if kind == 'internal':
        return SchNetAC(ObservationSpace(N, zs), ActionSpace(zs), (0.8, 1.8), 128, device='cuda:0')
    return CovariantAC(ObservationSpace(N, zs), ActionSpace(zs), bag_scale=cfg['bag_scale'], beta=cfg['beta'], device=torch.device('cuda'),
                       **MODEL_DEFAULTS)


def start_structure(N, n):
    """n atoms on a 1.6 lattice, S where all three indices are even, F elsewhere"""
    atoms = []
    for i in range(4):
        for j in range(3):
            for k in range(2):
                atoms.append((2 if (i % 2, j % 2, k % 2) == (0, 0, 0) else 1, (1.6 * i - 2.4, 1.6 * j - 1.6, 1.6 * k - 0.8)))
    return tuple(atoms[:n]) + ((0, (0.0, 0.0, 0.0)), ) * (N - n)


CONFIGURATIONS = [('CovariantAC, canvas 7', 'covariant', cfg['canvas_size'], [((16, 1), (9, 6))], None),
                  ('SchNetAC, canvas 7', 'internal', cfg['canvas_size'], [((16, 1), (9, 6))], None),
                  ('CovariantAC, canvas 40, 24-atom start', 'covariant', 40, [((16, 2), (9, 12))], 24)]


def measure(kind, N, formulas, start):
    ac = agent_of(kind, N)
    kw = dict(gamma=GAMMA, lam=LAM, min_reward=MIN_REWARD)
    if start is not None:
        kw['initial'] = (start_structure(N, start), (0, 12, 2))
    rolls = {'a': DeviceRollout(ac, formulas, E, steps, **kw)}
    if not only_a:
        from molgym_amd.rewards import PairReward
        R = PairReward(zs, EPS, SIGMA)
        rolls['b'] = DeviceRollout(ac, formulas, E, steps, reward_fn=R.host, **kw)
        rolls['c'] = DeviceRollout(ac, formulas, E, steps, reward=R, **kw)

    def collect(roll, seed):
        roll.reset()
        torch.manual_seed(seed)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        roll.collect(steps)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    times = {k: [] for k in rolls}
    with torch.no_grad():
        for roll in rolls.values():
            collect(roll, 0)  # warm-up
        same = None
        if not only_a:  # (b) and (c) recorded the same store
            vb, vc = rolls['b']._views(), rolls['c']._views()
            same = all(torch.equal(getattr(vb, name), getattr(vc, name)) for name in rolls['b']._table)
        for rep in range(repeats):
            for k, roll in rolls.items():
                times[k].append(collect(roll, 100 + rep))
    cut = None if only_a else int((rolls['c'].statuses() == 10).sum())
    return {k: (statistics.median(v) * 1e3, min(v) * 1e3, max(v) * 1e3) for k, v in times.items()}, same, cut


results = [(label, ) + measure(kind, N, formulas, start) for label, kind, N, formulas, start in CONFIGURATIONS]
if as_json:
    print(json.dumps({label: {k: v[0] / steps for k, v in ms.items()} for label, ms, _, _ in results}))
    sys.exit(0)
lines = [f'SF6-like formulas over zs {zs}, {E} environments x {steps} steps, min_reward {MIN_REWARD}; `collect` alone (reset outside '
         f'the timed region), median of {repeats} alternating repeats (fastest .. slowest), in ms.', '']
lines += ['| configuration | (a) `reward_fn=None` | (b) `reward_fn=R.host` | (c) `reward=R` | per step (a) / (b) / (c) | (c) - (a) per step | '
          '(b) - (a) per step | (b) and (c): same store | cuts in the last (c) |', '|---|---|---|---|---|---|---|---|---|']
for label, ms, same, cut in results:
    cell = lambda k: f'{ms[k][0]:.2f} ({ms[k][1]:.2f} .. {ms[k][2]:.2f})'
    if only_a:
        lines.append(f'| {label} | {cell("a")} | | | {ms["a"][0] / steps:.3f} | | | | |')
        continue
    lines.append(f'| {label} | {cell("a")} | {cell("b")} | {cell("c")} | {ms["a"][0] / steps:.3f} / {ms["b"][0] / steps:.3f} / '
                 f'{ms["c"][0] / steps:.3f} | {(ms["c"][0] - ms["a"][0]) / steps * 1e3:.0f} us | '
                 f'{(ms["b"][0] - ms["a"][0]) / steps * 1e3:.0f} us | {same} | {cut} |')
text = '\n'.join(lines) + '\n'
print(text)
if not only_a:
    with open(out_path, 'w') as f:
        f.write(text)
