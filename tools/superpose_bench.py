"""Measurement (GPU box): how far relaxed molecules moved -- the rigid superposition on the device against the host loop it replaces
  (s)  on the device   `superpose_canvases` on tensors that already lie there: one `mg_superpose`, synchronised
  (h)  on the host     both position tensors copied back, then a numpy SVD Kabsch (rmsd and rotation) in a Python loop over the pairs
  (r)  on the device   `relax(R, molecules, superpose=True)`: one upload, `mg_pair_relax`, `mg_superpose`, one copy back
  (rh) device + host   `relax(R, molecules)` and then the Kabsch loop over (input, relaxed)
  (d)  `relax(R, molecules)` at its default, for the comparison between two trees
for SF6 on a canvas of 7, 40 atoms on a canvas of 40 and 255 atoms on a canvas of 255 (jittered lattices, the Lennard-Jones
parameters of tools/relax_bench.py), 140 pairs each.  Every pair of columns is measured in alternating repeats -- (s) (h) (s) (h) ... --
and reported as the median with the fastest and the slowest.
usage: python tools/superpose_bench.py [num_molecules] [repeats] [out.md] [other_tree]
  other_tree: a built checkout of another commit (the parent).  (d) is then measured in fresh processes, three per tree,
  alternating, each of which prints one JSON line (`--default-relax TREE`); the table of their medians is added.
profiles/superpose.md holds the output with the notes added."""
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZS, EPS, SIGMA = [0, 9, 16], (0.0, 0.09, 0.12), (0.0, 1.40, 1.55)


def sf6(rng):
    axes = np.array([(1.0, 0, 0), (-1.0, 0, 0), (0, 1.0, 0), (0, -1.0, 0), (0, 0, 1.0), (0, 0, -1.0)])
    x = np.concatenate([np.zeros((1, 3)), 1.6 * axes]) + rng.normal(scale=0.08, size=(7, 3))
    return np.array([16] + [9] * 6), x


def lattice(n, shape):
    def make(rng):
        sites = np.array([(i, j, k) for i in range(shape[0]) for j in range(shape[1]) for k in range(shape[2])], dtype=np.float64)[:n]
        z = np.where((sites % 2 == 0).all(axis=1), 16, 9)
        return z, 1.6 * sites + rng.normal(scale=0.08, size=(n, 3))

    return make


CONFIGS = (('SF6, canvas 7', sf6), ('40 atoms, canvas 40', lattice(40, (4, 4, 3))), ('255 atoms, canvas 255', lattice(255, (7, 7, 6))))


def kabsch(a, b):
    a1, b1 = a - a.mean(axis=0), b - b.mean(axis=0)
    u, _, vt = np.linalg.svd(b1.T @ a1)
    rot = vt.T @ np.diag([1.0, 1.0, np.sign(np.linalg.det(vt.T @ u.T))]) @ u.T
    res = a1 - b1 @ rot.T
    return np.sqrt((res * res).sum() / len(a)), rot


def alternating(fns, repeats, sync):
    """the median, fastest and slowest ms of every function, measured in turn `repeats` times"""
    out = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            out[k].append((time.perf_counter() - t0) * 1e3)
    return [(statistics.median(v), min(v), max(v)) for v in out]


def default_relax(tree, E, repeats):
    """(d) in this process, with molgym_amd of `tree`: one JSON line"""
    sys.path.insert(0, tree)
    import torch
    import molgym_amd
    from molgym_amd import relax as X
    from molgym_amd.rewards import PairReward
    assert os.path.dirname(os.path.abspath(molgym_amd.__file__)) == os.path.join(os.path.abspath(tree), 'molgym_amd')
    R = PairReward(ZS, EPS, SIGMA)
    ms = {}
    for label, make in CONFIGS:
        rng = np.random.RandomState(0)
        mols = [make(rng) for _ in range(E)]
        X.relax(R, mols)
        ms[label] = alternating([lambda: X.relax(R, mols)], repeats, torch.cuda.synchronize)[0][0]
    print(json.dumps(dict(tree=os.path.abspath(tree), ms=ms)))


def main():
    argv = sys.argv[1:]
    if argv and argv[0] == '--default-relax':
        return default_relax(argv[1], int(argv[2]), int(argv[3]))
    E = int(argv[0]) if len(argv) > 0 else 140
    repeats = int(argv[1]) if len(argv) > 1 else 7
    out_path = argv[2] if len(argv) > 2 else None
    other = argv[3] if len(argv) > 3 else None
    sys.path.insert(0, HERE)
    import torch
    from molgym_amd import relax as X
    from molgym_amd import structure as S
    from molgym_amd.rewards import PairReward
    R = PairReward(ZS, EPS, SIGMA)
    cell = lambda v: f'{v[0]:.3f} ({v[1]:.3f} .. {v[2]:.3f})'
    lines = [f'{E} pairs per batch; median of {repeats} alternating repeats (fastest .. slowest), in ms per batch.', '',
             '| configuration | (s) `superpose_canvases` | (h) copy back + Kabsch loop | (h) / (s) | (r) `relax(superpose=True)` | (rh) `relax` + Kabsch loop | '
             '(rh) / (r) | (r) - `relax` | device and mirror: same bits | largest rmsd device - Kabsch | mean rmsd | mean displacement |',
             '|---|---|---|---|---|---|---|---|---|---|---|---|']
    for label, make in CONFIGS:
        rng = np.random.RandomState(0)
        mols = [make(rng) for _ in range(E)]
        N = len(mols[0][0])
        done = X.relax(R, mols, superpose=True)  # warm-up, and the result
        a, b = np.stack([x for _, x in mols]), np.stack([d.positions for d in done])
        d_a, d_b = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        natoms = torch.full((E, ), N, dtype=torch.int32, device='cuda')
        mirror = [S.superpose_host(a[e], b[e]) for e in range(min(E, 20))]
        same = all(d.rmsd == w.rmsd and d.displacement == w.displacement and d.max_deviation == w.max_deviation for d, w in zip(done, mirror))
        worst = max(abs(d.rmsd - kabsch(a[e], b[e])[0]) for e, d in enumerate(done))

        def host_loop(pa, pb):
            return [kabsch(pa[e], pb[e]) for e in range(E)]

        s, h = alternating([lambda: S.superpose_canvases(d_a, d_b, natoms), lambda: host_loop(d_a.cpu().numpy(), d_b.cpu().numpy())], repeats,
                           torch.cuda.synchronize)
        r, rh, plain = alternating([lambda: X.relax(R, mols, superpose=True),
                                    lambda: host_loop(a, np.stack([d.positions for d in X.relax(R, mols)])), lambda: X.relax(R, mols)], repeats,
                                   torch.cuda.synchronize)
        lines.append(f'| {label} | {cell(s)} | {cell(h)} | {h[0] / s[0]:.0f}x | {cell(r)} | {cell(rh)} | {rh[0] / r[0]:.1f}x | {r[0] - plain[0]:+.3f} | {same} | '
                     f'{worst:.1e} | {statistics.mean(d.rmsd for d in done):.4f} | {statistics.mean(d.displacement for d in done):.4f} |')
    if other:
        runs = {HERE: [], os.path.abspath(other): []}
        for _ in range(3):
            for tree in runs:
                got = subprocess.run([sys.executable, os.path.abspath(__file__), '--default-relax', tree, str(E), str(repeats)], check=True,
                                     stdout=subprocess.PIPE, timeout=300, cwd=tree)
                runs[tree].append(json.loads(got.stdout.decode().strip().splitlines()[-1])['ms'])
        lines += ['', f'`relax` at its default, ms per batch: three fresh processes per tree, alternating, each the median of {repeats} repeats.', '',
                  '| configuration | this tree | the other tree | spread between the processes of one tree |', '|---|---|---|---|']
        for label, _ in CONFIGS:
            mine, theirs = [m[label] for m in runs[HERE]], [m[label] for m in runs[os.path.abspath(other)]]
            spread = max(max(mine) - min(mine), max(theirs) - min(theirs))
            lines.append(f'| {label} | {" / ".join(f"{v:.3f}" for v in mine)} | {" / ".join(f"{v:.3f}" for v in theirs)} | {spread:.3f} |')
    text = '\n'.join(lines) + '\n'
    print(text)
    if out_path:
        with open(out_path, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
