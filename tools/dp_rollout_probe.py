"""Does the sampling launch give a row the same bits at batch E and at the batch of a rank's share?

The world invariance of a sharded `DeviceRollout` (profiles/dp_device_rollout.md) stands on it.  For both agents in training mode
a host loop steps 5 environments (the shapes of tests/test_gpu_dp_rollout.py: canvas 6, ZS [0, 1, 6, 8], H2O / CH4) for STEPS
steps; before every step the value-only launch `step_canvas(commit=False, seed, sample_ids)` runs on the canvas of all 5 and on
fresh canvases of the shares (2, 3) and (1, 2, 2), keyed `(lo, 1)`.  Action rows, logp, ent and v of every share are compared to
the rows `lo..hi` of the whole, bit for bit.  Uses only `make_canvas` / `step_canvas`, so it runs on any commit that has them.

usage: python tools/dp_rollout_probe.py [out.json]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from molgym_amd import ppo  # noqa: E402, F401
from tests.test_gpu_device_rollout import MIN_REWARD, SEED, PayingEnv, _seeds  # noqa: E402, F401
from tests.test_gpu_episodes import BAGS, CANVAS, MAX_SOLO, MIN_D, STEPS, ZS, _agent  # noqa: E402

E = 5
SPLITS = {2: ((0, 2), (2, 5)), 3: ((0, 1), (1, 3), (3, 5))}


def probe(kind, agent_seed):
    ac = _agent(kind, agent_seed)
    assert ac.training
    envs = [PayingEnv(CANVAS, ZS, BAGS, MIN_D, MAX_SOLO) for _ in range(E)]
    seeds = _seeds(SEED, STEPS)
    obs = [env._obs() for env in envs]
    cv = ac.make_canvas(obs)
    result = {f'world {w}': dict(launches=0, unequal=0, fields={}) for w in SPLITS}
    natoms_seen = set()
    with torch.no_grad():
        for t in range(STEPS):
            whole = ac.step_canvas(cv, commit=False, seed=seeds[t])
            natoms_seen.update(int(n) for n in cv.natoms)
            for w, shares in SPLITS.items():
                r = result[f'world {w}']
                for lo, hi in shares:
                    part = ac.step_canvas(ac.make_canvas(obs[lo:hi]), commit=False, seed=seeds[t], sample_ids=(lo, 1))
                    bad = [k for k in ('a', 'logp', 'ent', 'v') if not torch.equal(part[k], whole[k][lo:hi])]
                    if part['actions'] != whole['actions'][lo:hi]:
                        bad.append('actions')
                    r['launches'] += 1
                    r['unequal'] += bool(bad)
                    for k in bad:
                        r['fields'][k] = r['fields'].get(k, 0) + 1
            pred = ac.step_canvas(cv, seed=seeds[t])
            assert pred['actions'] == whole['actions'] and torch.equal(pred['logp'], whole['logp'])
            nxt, terminals = [], []
            for e, env in enumerate(envs):
                o, _, done, _ = env.step(pred['actions'][e])
                nxt.append(o)
                terminals.append(done)
            obs = [env.reset() if done else o for env, o, done in zip(envs, nxt, terminals)]
            stale = cv.stale_rows(obs, terminals)
            cv.sync(stale, [obs[i] for i in stale])
    result['atom counts met'] = sorted(natoms_seen)
    return result


def main():
    out = {f'{kind} (agent seed {s})': probe(kind, s) for kind, s in (('covariant', 0), ('internal', 5))}
    text = json.dumps(out, indent=1)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
