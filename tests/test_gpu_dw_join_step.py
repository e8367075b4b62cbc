"""The joined weight-gradient launch inside a CovariantAC PPO step (csrc/gemm_dispatch.inc: flush_dw, MG_DW_JOIN_WIDE).

The switches of the GEMM dispatchers are read once per process, so one tiny ppo_minibatch (5 canvases of 5, zs [0, 9, 16], model
defaults) runs in two fresh child interpreters: with the switch unset (the join) and with MG_DW_JOIN_WIDE=0 (the parent's launches).
The step with the join has one launch fewer -- the six 128-column layers no longer have a launch of their own -- the same loss
statistics (the forward and the loss are untouched), and a gradient that differs only by the grouping of the float32 partial sums of
those six layers: held to the gradient rule of tests/helpers.py (2e-4 of the slot maximum, 1e-2 relative above 1 % of it) against
the switch-off run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import helpers

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = '''
import json, sys
sys.path.insert(0, %r)
import numpy as np, torch
from molgym_amd.agents.covariant import CovariantAC
from molgym_amd.spaces import ActionSpace, ObservationSpace
from molgym_amd.synthetic import MODEL_DEFAULTS, make_batch
zs, canvas, B = [0, 9, 16], 5, 5
torch.manual_seed(3)
ac = CovariantAC(ObservationSpace(canvas, zs), ActionSpace(zs), bag_scale=5, beta=-10.0, device='cuda:0', **MODEL_DEFAULTS)
d = make_batch(B, canvas, zs, seed=4)
batch = ac.prepare_batch(d['obs'], d['act'], d['logp'], d['adv'], d['ret'])
stats = ac.ppo_minibatch(batch, 0.2, 0.5, 0.01)
torch.cuda.synchronize()
np.save(sys.argv[1], ac.theta.grad.cpu().numpy())
print(json.dumps({'launches': int(ac._L().mg_cov_step_launches()), 'graph': bool(ac.last_step_used_graph),
                  'stats': [float(v).hex() for v in stats.cpu()], 'slots': {k: [int(o), [int(x) for x in s]] for k, (o, s) in ac.slot_table.items()}}))
'''


def _run(tmp_path, name, switch):
    env = {k: v for k, v in os.environ.items() if k != 'MG_DW_JOIN_WIDE'}
    if switch is not None:
        env['MG_DW_JOIN_WIDE'] = switch
    path = str(tmp_path / f'{name}.npy')
    r = subprocess.run([sys.executable, '-c', _CHILD % ROOT, path], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1]), torch.from_numpy(np.load(path))


def test_join_takes_one_launch_off_the_step_and_keeps_the_results(built_lib, tmp_path):
    on, g_on = _run(tmp_path, 'join', None)
    off, g_off = _run(tmp_path, 'parent', '0')
    print('launches', on['launches'], off['launches'], 'max |grad diff| / max |grad|',
          ((g_on - g_off).abs().max() / g_off.abs().max()).item())
    assert on['graph'] and off['graph']
    assert on['launches'] == off['launches'] - 1
    assert on['stats'] == off['stats']
    assert torch.isfinite(g_on).all() and g_off.abs().max().item() > 0
    slots = {k: (o, tuple(s)) for k, (o, s) in off['slots'].items()}
    want = {k: helpers._Grad(g_off[o:o + int(np.prod(s))]) for k, (o, s) in slots.items()}
    helpers.assert_grads(helpers.grad_report(g_on, want, slots))
