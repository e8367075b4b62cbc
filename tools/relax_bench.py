"""Measurement (GPU box): relaxing a batch of molecules under a `PairReward` potential
  (a) on the device      `relax(R, molecules)`: one upload, one `mg_pair_relax`, one copy back
  (a') on the device     `relax_canvases` on tensors that already lie there: the launch alone
  (b) on the host        `relax_host` in a Python loop (the float64 mirror: same bits as (a))
  (c) scipy              the reference's call, `minimize(method='BFGS', jac=True, options=dict(maxiter=120, norm=inf, gtol=3e-4))`, on
                         the mirror's energy and gradient -- where scipy is importable
for SF6 (one S, six F on a jittered octahedron) on a canvas of 7, and for 40 atoms on a jittered 1.6 lattice on a canvas of 40, 140
molecules each, with the made-up Lennard-Jones parameters of tools/pair_reward_bench.py.  (b) and (c) run on the first `host_mols`
molecules and are scaled to the batch; median of the repeats with the fastest and the slowest.
usage: python tools/relax_bench.py [num_molecules] [repeats] [host_mols] [out.md]   (the table is printed; written to out.md if given --
profiles/relax.md holds it with the notes added)"""
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, '.')
from molgym_amd import relax as X  # noqa: E402
from molgym_amd.rewards import PairReward  # noqa: E402

argv = sys.argv[1:]
E = int(argv[0]) if len(argv) > 0 else 140
repeats = int(argv[1]) if len(argv) > 1 else 7
host_mols = min(E, int(argv[2]) if len(argv) > 2 else 20)
out_path = argv[3] if len(argv) > 3 else None
ZS, EPS, SIGMA = [0, 9, 16], (0.0, 0.09, 0.12), (0.0, 1.40, 1.55)
try:
    from scipy.optimize import minimize
except ImportError:
    minimize = None


def sf6(rng):
    axes = np.array([(1.0, 0, 0), (-1.0, 0, 0), (0, 1.0, 0), (0, -1.0, 0), (0, 0, 1.0), (0, 0, -1.0)])
    x = np.concatenate([np.zeros((1, 3)), 1.6 * axes]) + rng.normal(scale=0.08, size=(7, 3))
    return np.array([16] + [9] * 6), x


def lattice40(rng):
    sites = np.array([(i, j, k) for i in range(4) for j in range(4) for k in range(3)], dtype=np.float64)[:40]
    z = np.where((sites % 2 == 0).all(axis=1), 16, 9)
    return z, 1.6 * sites + rng.normal(scale=0.08, size=(40, 3))


def timed(fn, sync=False):
    out = []
    for _ in range(repeats):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def measure(make):
    R = PairReward(ZS, EPS, SIGMA)
    rng = np.random.RandomState(0)
    mols = [make(rng) for _ in range(E)]
    got = X.relax(R, mols)  # warm-up, and the result
    want = [X.relax_host(R, z, x) for z, x in mols[:host_mols]]
    same = all(g.positions.tobytes() == w.positions.tobytes() and (g.status, g.iterations, g.evaluations) == (w.status, w.iterations, w.evaluations)
               and g.energy == w.energy for g, w in zip(got, want))
    N = len(mols[0][0])
    pos = torch.from_numpy(np.stack([x for _, x in mols])).cuda()
    charges = torch.from_numpy(np.stack([z for z, _ in mols]).astype(np.int32)).cuda()
    natoms = torch.full((E, ), N, dtype=torch.int32, device='cuda')
    ms = {'a': timed(lambda: X.relax(R, mols), sync=True), 'k': timed(lambda: X.relax_canvases(R, pos, charges, natoms), sync=True),
          'b': timed(lambda: [X.relax_host(R, z, x) for z, x in mols[:host_mols]])}
    ref = None
    if minimize is not None:

        def bfgs(z, x):
            f = lambda v: (lambda e, g, _: (e, g.reshape(-1)))(*R.energy_forces(z, v.reshape(-1, 3)))
            return minimize(f, x.reshape(-1), jac=True, method='BFGS', options=dict(maxiter=120, norm=np.inf, gtol=3e-4))

        ref = [bfgs(z, x) for z, x in mols[:host_mols]]
        ms['c'] = timed(lambda: [bfgs(z, x) for z, x in mols[:host_mols]])
    hist = [sum(g.status == s for g in got) for s in range(4)]
    iters = statistics.mean(g.iterations for g in got)
    drop = statistics.mean(g.energy_before - g.energy for g in got)
    agree = None if ref is None else sum(r.success and w.success and abs(r.fun - w.energy) <= 1e-6 for r, w in zip(ref, want))
    return ms, same, hist, iters, drop, agree, None if ref is None else sum(bool(r.success) for r in ref)


results = [(label, ) + measure(make) for label, make in (('SF6, canvas 7', sf6), ('40 atoms, canvas 40', lattice40))]
scale = E / host_mols
cell = lambda v, f=1.0: f'{v[0] * f:.2f} ({v[1] * f:.2f} .. {v[2] * f:.2f})'
lines = [f'{E} molecules per batch, max_iter 120, gtol 3e-4; median of {repeats} repeats (fastest .. slowest), in ms per batch.  (b) and (c) ran '
         f'on the first {host_mols} molecules and are scaled by {scale:g}.', '',
         '| configuration | (a) `relax` | (a\') `relax_canvases` | (b) `relax_host` loop | (c) scipy BFGS on the mirror | (b) / (a) | (c) / (a) | '
         '(a) and (b): same bits | CONVERGED / MAX_ITER / LINE_SEARCH / NONFINITE | mean iterations | mean energy drop | '
         f'scipy succeeded, of {host_mols} | both succeeded within 1e-6, of {host_mols} |', '|---|---|---|---|---|---|---|---|---|---|---|---|---|']
for label, ms, same, hist, iters, drop, agree, ok in results:
    c = cell(ms['c'], scale) if 'c' in ms else 'no scipy'
    rc = f'{ms["c"][0] * scale / ms["a"][0]:.0f}x' if 'c' in ms else ''
    lines.append(f'| {label} | {cell(ms["a"])} | {cell(ms["k"])} | {cell(ms["b"], scale)} | {c} | {ms["b"][0] * scale / ms["a"][0]:.0f}x | {rc} | {same} | '
                 f'{" / ".join(str(h) for h in hist)} | {iters:.1f} | {drop:.4f} | {ok} | {agree} |')
text = '\n'.join(lines) + '\n'
print(text)
if out_path:
    with open(out_path, 'w') as f:
        f.write(text)
