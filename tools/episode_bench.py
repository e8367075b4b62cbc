"""Measurement (GPU box): environment steps/s and finished molecules/s of `DeviceEpisodes.run` against the serial canvas
rollout (`ppo.batch_rollout` on `step_canvas`) over the host rules environment of the tests (tests/episode_ref.py: the same
rules, zero reward).  Same agent, same seeds, SF6 (BASELINE configs[1]: zs [0, 9, 16], canvas 7), 140 environments; the two
alternate in one process and the median of the repeats is reported (with the fastest and slowest repeat of the device loop).
(`run(seed=s)` derives its per-step seeds as `torch.manual_seed(s)` + `draw_seed()` does, so both loops draw the same actions.)
The fifth argument selects the rule set; SF6 itself fits none of the other three (it fills the canvas, holds the only possible
scaffold element and sulfur has no bond count), so each takes the nearest workload on the same zs and canvas:
  default   MolecularEnvironment, SF6 (mg_episode_step)
  refill    RefillableMolecularEnvironment: SF2 then F2, num_refills = 2 (up to SF6 on the canvas of 7)
  hull      ConstrainedMolecularEnvironment: a tetrahedron of four S as the scaffold, F3 to place inside it
  sampled   StochasticEnvironment: formulas drawn from F6 with sizes in [2, 7)
usage: python tools/episode_bench.py [num_envs] [steps] [repeats] [covariant|internal] [default|refill|hull|sampled]"""
import statistics
import sys
import time

import torch

sys.path.insert(0, '.')
from molgym_amd import ppo  # noqa: E402
from molgym_amd.buffer import PPOBufferContainer  # noqa: E402
from molgym_amd.env_container import SimpleEnvContainer  # noqa: E402
from molgym_amd.episodes import DeviceEpisodes  # noqa: E402
from molgym_amd.spaces import ActionSpace, ObservationSpace  # noqa: E402
from molgym_amd.synthetic import CONFIGS, MODEL_DEFAULTS  # noqa: E402
from tests.episode_ref import RulesEnv  # noqa: E402

E = int(sys.argv[1]) if len(sys.argv) > 1 else 140
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 28
repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 7
kind = sys.argv[4] if len(sys.argv) > 4 else 'covariant'
rules = sys.argv[5] if len(sys.argv) > 5 else 'default'
cfg = CONFIGS['cfg2']
zs, N = cfg['zs'], cfg['canvas_size']
TETRA = tuple((zs.index(16), p) for p in ((1.6, 1.6, 1.6), (1.6, -1.6, -1.6), (-1.6, 1.6, -1.6), (-1.6, -1.6, 1.6)))
# rule set -> formulas, their bags, start structure, DeviceEpisodes keywords
WORKLOADS = {
    'default': ([((16, 1), (9, 6))], [(0, 6, 1)], (), {}),  # SF6
    'refill': ([((16, 1), (9, 2)), ((9, 2), )], [(0, 2, 1), (0, 2, 0)], (), dict(num_refills=2)),
    'hull': ([((9, 3), )], [(0, 3, 0)], TETRA, dict(scaffold_z=16)),
    'sampled': ([((9, 6), )], [(0, 6, 0)], (), dict(size_range=(2, 7))),
}
formulas, bags, start, rule_kw = WORKLOADS[rules]
initial = None if not start else (start + ((0, (0.0, 0.0, 0.0)), ) * (N - len(start)), bags[0])
torch.manual_seed(0)
if kind == 'covariant':
    from molgym_amd.agents.covariant import CovariantAC
    ac = CovariantAC(ObservationSpace(N, zs), ActionSpace(zs), bag_scale=cfg['bag_scale'], beta=cfg['beta'],
                     device=torch.device('cuda'), **MODEL_DEFAULTS)
else:
    from molgym_amd.agents.internal import SchNetAC
    ac = SchNetAC(ObservationSpace(N, zs), ActionSpace(zs), (0.8, 1.8), 128, device=torch.device('cuda'))
    ac.rollout_on_canvas = True


def host_envs():
    if rules == 'default':
        return [RulesEnv(N, zs, bags) for _ in range(E)]
    from tests.episode_rules_ref import RulesEnvX
    kw = dict(start=start, num_refills=rule_kw.get('num_refills', 0), scaffold_z=rule_kw.get('scaffold_z'))
    if rules == 'sampled':  # (one key per environment for the whole run: the host loop is here for its time alone)
        lo, hi = rule_kw['size_range']
        kw['sampler'] = dict(counts=bags[0], size_min=lo, size_max=hi, max_tries=64)
    # batch_rollout resets every environment once more before its first step, which moves a formula cycle on by one: the host
    # environments get the cycle rotated back, so that both loops start on formulas[0]
    return [RulesEnvX(N, zs, bags[-1:] + bags[:-1], draw_key=(0, e), **kw) for e in range(E)]


def host_loop(seed):
    envs = host_envs()
    container = PPOBufferContainer(size=E, gamma=0.99, lam=0.97)
    torch.manual_seed(seed)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ppo.batch_rollout(ac, SimpleEnvContainer(envs), container, num_steps=E * steps)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, sum(env.episode for env in envs) - E  # (batch_rollout resets every environment once first)


def device_loop(seed):
    eps = DeviceEpisodes(ac, formulas, E, initial=initial, **rule_kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    done = eps.run(num_steps=steps, seed=seed)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, len(done)


host_loop(0), device_loop(0)  # warm-up: workspaces, first launches
rows = {'host': [], 'device': []}
for rep in range(repeats):
    rows['host'].append(host_loop(100 + rep))
    rows['device'].append(device_loop(100 + rep))
print(f'{kind}, {rules} rules, formulas {formulas}, canvas {N}, {E} environments x {steps} steps, median of {repeats} alternating repeats')
med = {}
for name, label in (('host', 'batch_rollout (step_canvas + host rules environments)'), ('device', 'DeviceEpisodes.run')):
    dt = statistics.median(t for t, _ in rows[name])
    mols = statistics.median(m for _, m in rows[name])
    med[name] = dt
    print(f'{label}: {dt * 1e3:.1f} ms, {dt / steps * 1e3:.3f} ms per step of all environments, {E * steps / dt:.0f} environment '
          f'steps/s, {mols / dt:.0f} finished molecules/s ({mols:.0f} molecules)')
dev = sorted(t for t, _ in rows['device'])
print(f'DeviceEpisodes.run repeats: fastest {dev[0] * 1e3:.1f} ms, slowest {dev[-1] * 1e3:.1f} ms')
print(f'ratio host / device: {med["host"] / med["device"]:.2f}')
