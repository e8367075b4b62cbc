"""`mg_pair_energy_forces` and `mg_pair_relax` against their float64 host mirrors (`PairReward.energy_forces`, `relax_host` of
molgym_amd/relax.py): every comparison is `np.array_equal` -- float64 `/` is correctly rounded on the device, contraction is off
and both sides state one operation order (NaN compares equal to NaN: the sign and payload of a NaN are not part of the contract,
x86 and the device produce different ones).  Then `relax` on sampled molecules and `relax_canvases` on a resident canvas.

The clusters: n sites of a 7 x 7 x 7 lattice of spacing 1.12 with a normal jitter of sigma 0.05, nearest to one corner first, three
elements whose six eps_ij and six sigma_ij all differ.  Slots beyond a row's atoms hold NaN positions and the charge 99."""
import ctypes as C

import numpy as np
import pytest
import torch

from molgym_amd import _lib
from molgym_amd import relax as X
from molgym_amd.rewards import PairReward

pytestmark = pytest.mark.gpu
GUARD = 4096
K_ZS = [1, 6, 8]
K_EPS = np.array([[0.50, 0.71, 0.93], [0.71, 1.10, 1.27], [0.93, 1.27, 1.60]])
K_SIGMA = np.array([[0.90, 0.97, 0.93], [0.97, 1.04, 1.01], [0.93, 1.01, 0.98]])
CUTOFF = 2.6
_CACHE = {}


def potential(cutoff=None):
    return PairReward(K_ZS, K_EPS, K_SIGMA, cutoff=cutoff)


def canvases(N, counts, seed, fixed_every=0):
    """(pos [E][N][3], charges [E][N], natoms [E], fixed [E][N] uint8) with poisoned slots beyond the atoms"""
    rng = np.random.RandomState(seed)
    sites = np.array([(i, j, k) for i in range(7) for j in range(7) for k in range(7)], dtype=np.float64) * 1.12
    sites = sites[np.argsort(np.linalg.norm(sites, axis=1), kind='stable')]
    E = len(counts)
    pos, charges = np.full((E, N, 3), np.nan), np.full((E, N), 99, dtype=np.int32)
    fixed = np.zeros((E, N), dtype=np.uint8)
    for e, n in enumerate(counts):
        pos[e, :n] = sites[:n] + rng.normal(scale=0.05, size=(n, 3))
        charges[e, :n] = rng.choice(K_ZS, size=n)
        if fixed_every:
            fixed[e, e % fixed_every:n:fixed_every] = 1
            fixed[e, n:] = 1  # (a mask beyond the atoms is not looked at)
    return pos, charges, np.array(counts, dtype=np.int32), fixed


class _Guarded:
    """a device array with the bytes of the host array `init`, between two guard bands of 0xA5"""

    def __init__(self, init):
        host = torch.from_numpy(np.ascontiguousarray(init))
        self.nbytes = host.numel() * host.element_size()
        self.big = torch.full((GUARD + self.nbytes + GUARD, ), 0xA5, dtype=torch.uint8, device='cuda')
        self.t = self.big[GUARD:GUARD + self.nbytes].view(host.dtype).view(host.shape)
        self.t.copy_(host)

    def intact(self):
        return bool((self.big[:GUARD] == 0xA5).all()) and bool((self.big[GUARD + self.nbytes:] == 0xA5).all())

    def host(self):
        return self.t.cpu().numpy()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _common(R, N, E, d, fixed, override=None):
    four_eps, sigma2 = R.device_tables(torch.device('cuda:0'))
    a = dict(E=E, N=N, Z=len(K_ZS), cutoff2=R.cutoff2)
    a.update(override or {})
    return (a['E'], a['N'], a['Z'], (C.c_int32 * len(K_ZS))(*K_ZS), _p(four_eps), _p(sigma2), a['cutoff2'], _p(d['pos']), _p(d['charges']),
            _p(d['natoms']), _p(d['fixed']) if fixed else None)


def _upload(case):
    pos, charges, natoms, fixed = case
    return dict(pos=torch.from_numpy(pos).cuda(), charges=torch.from_numpy(charges).cuda(), natoms=torch.from_numpy(natoms).cuda(),
                fixed=torch.from_numpy(fixed).cuda())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ---- 1. mg_pair_energy_forces ----------------------------------------------------------------------------------------------------
EF_CASES = {
    '7': (7, [0, 1, 2, 7, 5]), '70': (70, [63, 64, 65, 70, 2]), '255': (255, [255, 65, 0, 1, 64]), '7x1': (7, [7]), '255x1': (255, [255]),
}


@pytest.mark.parametrize('cutoff', [None, CUTOFF])
@pytest.mark.parametrize('fixed', [False, True])
@pytest.mark.parametrize('name', list(EF_CASES))
def test_energy_forces_against_the_host_mirror(built_lib, name, fixed, cutoff):
    N, counts = EF_CASES[name]
    case = canvases(N, counts, seed=N + len(counts), fixed_every=3 if fixed else 0)
    pos, charges, natoms, fx = case
    R, E = potential(cutoff), len(counts)
    d = _upload(case)
    out = (_Guarded(np.full(E, -777.0)), _Guarded(np.full((E, N, 3), -777.0)), _Guarded(np.full(E, -777.0)))
    rc = built_lib.mg_pair_energy_forces(*_common(R, N, E, d, fixed), _p(out[0].t), _p(out[1].t), _p(out[2].t), _stream())
    torch.cuda.synchronize()
    assert rc == 0, built_lib.mg_last_error()
    assert all(o.intact() for o in out)
    energy, grad, gmax = (o.host() for o in out)
    dropped = 0
    for e, n in enumerate(counts):
        mask = fx[e, :n].astype(bool) if fixed else None
        wE, wg, wmax = R.energy_forces(charges[e, :n], pos[e, :n], mask)
        print(name, 'row', e, 'n', n, 'E', energy[e], 'gmax', gmax[e])
        assert energy[e] == wE and gmax[e] == wmax and np.array_equal(grad[e, :n], wg), (e, n)
        assert not grad[e, n:].any() and not np.signbit(grad[e, n:]).any()
        if fixed and n:
            assert not grad[e, :n][mask].any() and (n < 2 or grad[e, :n][~mask].all())
        assert np.isfinite(wE) and (wmax > 0.0) == (n >= 2)
        r = np.linalg.norm(pos[e, :n, None] - pos[e, None, :n], axis=2)
        dropped += int((r > CUTOFF).sum())
    assert dropped > 0 or N == 7
    for k, t in d.items():  # the inputs are inputs
        assert _same(t.cpu().numpy(), case[('pos', 'charges', 'natoms', 'fixed').index(k)]), k


def test_energy_forces_rows_that_cannot_be_evaluated(built_lib):
    """a coincident pair and a charge outside zs give NaN; an atom count outside 0 .. N gives NaN, a +0.0 gradient and reads nothing"""
    N, counts = 7, [4, 5, 3, 6, 2]
    case = canvases(N, counts, seed=1)
    pos, charges, natoms, fx = case
    pos[0, 3] = pos[0, 1]
    charges[1, 2] = 9
    natoms[2], natoms[3] = N + 1, -1
    R, E = potential(), len(counts)
    d = _upload(case)
    out = (_Guarded(np.full(E, -777.0)), _Guarded(np.full((E, N, 3), -777.0)), _Guarded(np.full(E, -777.0)))
    assert built_lib.mg_pair_energy_forces(*_common(R, N, E, d, False), _p(out[0].t), _p(out[1].t), _p(out[2].t), _stream()) == 0
    torch.cuda.synchronize()
    energy, grad, gmax = (o.host() for o in out)
    assert all(o.intact() for o in out)
    for e in (0, 1, 4):
        wE, wg, wmax = R.energy_forces(charges[e, :counts[e]], pos[e, :counts[e]])
        assert _same(energy[e], wE) and _same(grad[e, :counts[e]], wg) and _same(gmax[e], wmax)
    assert np.isnan(energy[:4]).all() and np.isnan(gmax[:4]).all() and np.isfinite(energy[4])
    assert not grad[2:4].any() and not np.signbit(grad[2:4]).any()


# ---- 2. mg_pair_relax ------------------------------------------------------------------------------------------------------------
def _relax_launch(lib, R, N, E, d, fixed, max_iter=120, gtol=3e-4, alias=False, override=None):
    """one mg_pair_relax into guarded outputs and a guarded scratch of exactly the reported size -> (rc, outputs, all intact)"""
    out_pos = None if alias else _Guarded(np.full((E, N, 3), -777.0))
    f = [_Guarded(np.full(E, -777.0)) for _ in range(3)]
    i = [_Guarded(np.full(E, -7, dtype=np.int32)) for _ in range(3)]
    nbytes = int(lib.mg_pair_relax_scratch_bytes(E, N))
    scratch = _Guarded(np.zeros(nbytes, dtype=np.uint8))
    rc = lib.mg_pair_relax(*_common(R, N, E, d, fixed, override), max_iter, gtol, _p(d['pos'] if alias else out_pos.t), *[_p(o.t) for o in f + i],
                           _p(scratch.t) if nbytes else None, nbytes, _stream())
    torch.cuda.synchronize()
    intact = all(o.intact() for o in f + i + [scratch] + ([] if alias else [out_pos]))
    got = dict(positions=(d['pos'] if alias else out_pos.t).cpu().numpy(), energy_before=f[0].host(), energy=f[1].host(), max_gradient=f[2].host(),
               iterations=i[0].host(), evaluations=i[1].host(), status=i[2].host())
    return rc, got, intact


def _mirror(R, case, fixed, max_iter=120, gtol=3e-4):
    pos, charges, natoms, fx = case
    return [X.relax_host(R, charges[e, :n], pos[e, :n], fx[e, :n].astype(bool) if fixed else None, max_iter, gtol) for e, n in enumerate(natoms)]


def _assert_rows(got, want, case, rows=None):
    pos, natoms = case[0], case[2]
    for e in (range(len(want)) if rows is None else rows):
        n, w = int(natoms[e]), want[e]
        print('row', e, 'n', n, X.STATUS_NAMES[w.status], 'iterations', w.iterations, 'evaluations', w.evaluations, 'E', w.energy_before, '->', w.energy)
        assert got['status'][e] == w.status and got['iterations'][e] == w.iterations and got['evaluations'][e] == w.evaluations, e
        assert _same(got['energy_before'][e], w.energy_before) and _same(got['energy'][e], w.energy) and _same(got['max_gradient'][e], w.max_gradient), e
        assert got['positions'][e, :n].tobytes() == w.positions.tobytes(), e
        assert got['positions'][e, n:].tobytes() == pos[e, n:].tobytes(), e  # slots beyond the atoms: the input's bytes


def _mixed():
    if 'mixed' not in _CACHE:
        R = potential(CUTOFF)
        case = canvases(255, [0, 1, 2, 7, 65, 255], seed=11)
        _CACHE['mixed'] = (R, case, _mirror(R, case, False))
    return _CACHE['mixed']


def test_relax_one_launch_of_mixed_sizes(built_lib):
    R, case, want = _mixed()
    d = _upload(case)
    rc, got, intact = _relax_launch(built_lib, R, 255, 6, d, False)
    assert rc == 0 and intact, built_lib.mg_last_error()
    _assert_rows(got, want, case)
    status = [w.status for w in want]
    assert status[:4] == [X.CONVERGED] * 4 and [w.iterations for w in want[:2]] == [0, 0] and want[2].iterations > 0 and want[3].iterations > 8
    assert all(s in (X.CONVERGED, X.MAX_ITER) for s in status[4:]) and all(w.energy < w.energy_before for w in want[2:])
    assert _same(d['pos'].cpu().numpy(), case[0])


def test_relax_into_its_own_input(built_lib):
    R, case, want = _mixed()
    d = _upload(case)
    rc, got, intact = _relax_launch(built_lib, R, 255, 6, d, False, alias=True)
    assert rc == 0 and intact
    _assert_rows(got, want, case)


@pytest.mark.parametrize('max_iter', [0, 1])
def test_relax_iteration_limits(built_lib, max_iter):
    R = potential()
    case = canvases(70, [2, 7, 64, 70, 0], seed=5)
    want = _mirror(R, case, False, max_iter=max_iter)
    rc, got, intact = _relax_launch(built_lib, R, 70, 5, _upload(case), False, max_iter=max_iter)
    assert rc == 0 and intact
    _assert_rows(got, want, case)
    assert [w.status for w in want] == [X.MAX_ITER] * 4 + [X.CONVERGED] and [w.iterations for w in want] == [max_iter] * 4 + [0]
    if max_iter == 0:
        assert _same(got['positions'], case[0])


def test_relax_with_fixed_atoms(built_lib):
    R = potential()
    case = canvases(7, [7, 6, 3, 2, 7], seed=9, fixed_every=2)
    case[3][4, :7] = 1  # every atom of the last row
    case[0][0, 0, 0] = -0.0
    want = _mirror(R, case, True)
    rc, got, intact = _relax_launch(built_lib, R, 7, 5, _upload(case), True)
    assert rc == 0 and intact
    _assert_rows(got, want, case)
    fx = case[3].astype(bool)
    assert got['positions'][fx].tobytes() == case[0][fx].tobytes()
    assert (want[4].status, want[4].iterations, want[4].max_gradient) == (X.CONVERGED, 0, 0.0) and all(w.iterations > 0 for w in want[:4])
    # and without the mask the same rows move
    rc, free, intact = _relax_launch(built_lib, R, 7, 5, _upload(case), False)
    assert rc == 0 and intact and (free['positions'][4] != case[0][4]).all()


def test_relax_rows_that_cannot_be_relaxed(built_lib):
    """coincident atoms and a charge outside zs: NONFINITE by the mirror too, positions the input's bytes; an atom count outside
    0 .. N: NONFINITE, NaN energies, nothing evaluated, the row copied; the rows between them relax as if alone"""
    N, counts = 7, [4, 5, 3, 6, 7]
    case = canvases(N, counts, seed=2)
    pos, charges, natoms, fx = case
    pos[0, 3] = pos[0, 1]
    charges[1, 2] = 9
    R = potential()
    want = _mirror(R, case, False)
    natoms[2], natoms[3] = N + 1, -1
    rc, got, intact = _relax_launch(built_lib, R, N, 5, _upload(case), False)
    assert rc == 0 and intact
    _assert_rows(got, want, case, rows=(0, 1, 4))
    assert [want[0].status, want[1].status, want[4].status] == [X.NONFINITE, X.NONFINITE, X.CONVERGED]
    for e in (2, 3):
        assert (got['status'][e], got['iterations'][e], got['evaluations'][e]) == (X.NONFINITE, 0, 0)
        assert np.isnan([got['energy_before'][e], got['energy'][e], got['max_gradient'][e]]).all()
    assert got['positions'][:4].tobytes() == pos[:4].tobytes()


def test_entry_points_refuse_bad_arguments(built_lib):
    R, N, E = potential(), 7, 5
    case = canvases(N, [7, 6, 3, 2, 7], seed=9)
    d = _upload(case)
    bad = [dict(E=0), dict(N=0), dict(N=256), dict(Z=1), dict(Z=17), dict(cutoff2=0.0), dict(cutoff2=float('nan')), dict(E=1 << 23, N=255)]
    for override in bad:
        assert _relax_launch(built_lib, R, N, E, d, False, override=override)[0] == -1, override
        out = torch.zeros(E * N * 3 + 2 * E, dtype=torch.float64, device='cuda')
        assert built_lib.mg_pair_energy_forces(*_common(R, N, E, d, False, override), _p(out), _p(out), _p(out), _stream()) == -1, override
    for kw in (dict(max_iter=-1), dict(gtol=-1e-3), dict(gtol=float('nan')), dict(gtol=float('inf'))):
        assert _relax_launch(built_lib, R, N, E, d, False, **kw)[0] == -1, kw
    args = list(_common(R, N, E, d, False))
    p, s = _p(torch.zeros(E * N * 3, dtype=torch.float64, device='cuda')), _stream()
    for k in (3, 4, 5, 7, 8, 9):  # zs_host, the tables, positions, charges, atom counts
        a = [None if i == k else v for i, v in enumerate(args)]
        assert built_lib.mg_pair_energy_forces(*a, p, p, p, s) == -1 and built_lib.mg_pair_relax(*a, 1, 1e-3, *[p] * 7, None, 0, s) == -1, k
    for k in range(7):
        outs = [None if i == k else p for i in range(7)]
        assert built_lib.mg_pair_relax(*args, 1, 1e-3, *outs, None, 0, s) == -1, k
    for k in range(3):
        outs = [None if i == k else p for i in range(3)]
        assert built_lib.mg_pair_energy_forces(*args, *outs, s) == -1, k
    torch.cuda.synchronize()


# ---- 3. relax and relax_canvases --------------------------------------------------------------------------------------------------
ZS4, A_EPS, A_SIGMA = [0, 1, 6, 8], (0.0, 0.08, 0.10, 0.12), (0.0, 1.35, 1.45, 1.40)
FORMULAS = [((6, 1), (1, 4)), ((1, 2), (8, 1)), ((6, 1), (8, 2))]


def _agent():
    if 'agent' not in _CACHE:
        from tests.test_gpu_episodes_env import _agent as agent_of
        _CACHE['agent'] = agent_of('internal', 1, ZS4, 7)
    return _CACHE['agent']


def _assert_relaxed(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert (g.status, g.iterations, g.evaluations, g.success) == (w.status, w.iterations, w.evaluations, w.success)
        assert _same(g.energy_before, w.energy_before) and _same(g.energy, w.energy) and _same(g.max_gradient, w.max_gradient)
        assert g.positions.shape == w.positions.shape and g.positions.tobytes() == w.positions.tobytes()


def test_relax_of_sampled_molecules_equals_the_mirror(built_lib):
    from molgym_amd.episodes import sample_molecules
    R = PairReward(ZS4, A_EPS, A_SIGMA)
    mols = sample_molecules(_agent(), FORMULAS, 8, num_envs=4, seed=3, min_atomic_distance=1.0)
    sizes = [len(m.numbers) for m in mols]
    print('sizes', sizes)
    assert len(mols) == 8 and max(sizes) >= 3 and len(set(sizes)) > 1
    got = X.relax(R, mols)
    want = [X.relax_host(R, m.numbers, m.positions) for m in mols]
    _assert_relaxed(got, want)
    print([(X.STATUS_NAMES[w.status], w.iterations) for w in want])
    assert any(w.iterations > 0 and w.energy < w.energy_before for w in want)
    # pairs instead of episodes, one list of fixed atoms for all, one per molecule
    big = [(m.numbers, m.positions) for m in mols if len(m.numbers) >= 2]
    _assert_relaxed(X.relax(R, big, fixed_indices=[1]), [X.relax_host(R, z, x, fixed=[1]) for z, x in big])
    per = [[0] if k % 2 else [] for k in range(len(big))]
    _assert_relaxed(X.relax(R, big, fixed_indices=per, max_iter=3), [X.relax_host(R, z, x, fixed=f, max_iter=3) for (z, x), f in zip(big, per)])


def test_relax_canvases_on_a_resident_canvas_equals_relax(built_lib):
    from molgym_amd.episodes import DeviceEpisodes
    R = PairReward(ZS4, A_EPS, A_SIGMA)
    from tests.test_gpu_episodes_env import WATER
    start = tuple(WATER) + ((0, (0.0, 0.0, 0.0)), ) * 4  # every episode starts from a water molecule: three atoms or more per canvas
    eps = DeviceEpisodes(_agent(), FORMULAS, 6, initial=(start, (0, 4, 1, 0)), min_atomic_distance=1.0)
    eps.run(num_steps=3, seed=5)
    cv = eps.canvas
    pos, charges, natoms = cv.pos64.cpu().numpy(), cv.charges.cpu().numpy(), cv.natoms_dev.cpu().numpy()
    print('atoms on the canvases', natoms)
    assert natoms.min() >= 3 and np.array_equal(natoms, cv.natoms)
    mols = [(charges[e, :n], pos[e, :n]) for e, n in enumerate(natoms)]
    want = X.relax(R, mols)
    got = X.relax_canvases(R, cv.pos64, cv.charges, cv.natoms_dev)
    assert all(t.is_cuda for t in got.values()) and torch.equal(cv.pos64.cpu(), torch.from_numpy(pos))
    assert any(w.iterations > 0 and w.energy < w.energy_before for w in want)
    for e, (n, w) in enumerate(zip(natoms, want)):
        assert got['positions'][e, :n].cpu().numpy().tobytes() == w.positions.tobytes() and torch.equal(got['positions'][e, n:], cv.pos64[e, n:])
        assert (int(got['status'][e]), int(got['iterations'][e]), int(got['evaluations'][e])) == (w.status, w.iterations, w.evaluations)
        assert _same(float(got['energy_before'][e]), w.energy_before) and _same(float(got['energy'][e]), w.energy)
        assert _same(float(got['max_gradient'][e]), w.max_gradient)
    ef = X.energy_forces_canvases(R, cv.pos64, cv.charges, cv.natoms_dev)
    assert _same(ef['energy'].cpu().numpy(), np.array([w.energy_before for w in want]))
    for e, n in enumerate(natoms):
        assert np.array_equal(ef['grad'][e, :n].cpu().numpy(), R.energy_forces(charges[e, :n], pos[e, :n])[1])
    # in place: the canvas itself takes the relaxed positions
    work = cv.pos64.clone()
    assert X.relax_canvases(R, work, cv.charges, cv.natoms_dev, out=work)['positions'] is work and torch.equal(work, got['positions'])
