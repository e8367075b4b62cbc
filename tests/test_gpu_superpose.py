"""`mg_superpose` against its float64 host mirror (`superpose_host` of molgym_amd/structure.py): every comparison is
`np.array_equal(..., equal_nan=True)` or bytes -- float64 `/` and `sqrt` are correctly rounded on the device, contraction is off and
both sides state one operation order (NaN compares equal to NaN: the sign and payload of a computed NaN are not part of the
contract).  Then `superpose` and `superpose_canvases`, and `relax` / `relax_canvases` with `superpose=True`.

The pairs: A is a cluster of tests/test_gpu_relax.py::canvases, B the same cluster jittered by 0.05, turned and shifted
(tests/test_superpose_host.py::moved).  Slots beyond a row's atoms hold NaN in both; the mask, where there is one, switches every
third atom off and is set beyond the atoms, where it must not be read."""
import ctypes as C

import numpy as np
import pytest
import torch

from molgym_amd import relax as X
from molgym_amd import structure as S
from molgym_amd.rewards import PairReward
from tests.test_gpu_relax import A_EPS, A_SIGMA, EF_CASES, FORMULAS, ZS4, _agent, _Guarded, _p, _same, _stream, canvases
from tests.test_superpose_host import moved

pytestmark = pytest.mark.gpu
FIELDS = ('rmsd', 'displacement', 'max_deviation', 'rotation', 'centroid_a', 'centroid_b', 'status')
_CACHE = {}


def pairs(name):
    """(a [E][N][3], b [E][N][3], natoms [E], select [E][N] uint8) and the mirror's rows with and without the mask, computed once"""
    if name not in _CACHE:
        N, counts = EF_CASES[name]
        a, _, natoms, _ = canvases(N, counts, seed=40 + N + len(counts))
        b = np.full_like(a, np.nan)
        select = np.ones((len(counts), N), dtype=np.uint8)
        for e, n in enumerate(counts):
            b[e, :n] = moved(a[e, :n], 0.05, seed=7 * N + e)
            select[e, (e % 3):n:3] = 0
        want = {masked: [S.superpose_host(a[e, :n], b[e, :n], select[e, :n].astype(bool) if masked else None) for e, n in enumerate(counts)]
                for masked in (False, True)}
        _CACHE[name] = (a, b, natoms, select, want)
    return _CACHE[name]


def launch(lib, a, b, natoms, select=None, alias=False, no_aligned=False, override=None):
    """one mg_superpose into guarded outputs -> (rc, outputs, all guard bands intact, the device inputs)"""
    E, N = a.shape[:2]
    d = dict(a=torch.from_numpy(a).cuda(), b=torch.from_numpy(b).cuda(), natoms=torch.from_numpy(natoms).cuda(),
             select=None if select is None else torch.from_numpy(select).cuda())
    aligned = None if alias or no_aligned else _Guarded(np.full((E, N, 3), -777.0))
    out = dict(rmsd=_Guarded(np.full(E, -777.0)), displacement=_Guarded(np.full(E, -777.0)), max_deviation=_Guarded(np.full(E, -777.0)),
               rotation=_Guarded(np.full((E, 9), -777.0)), centroid_a=_Guarded(np.full((E, 3), -777.0)),
               centroid_b=_Guarded(np.full((E, 3), -777.0)), status=_Guarded(np.full(E, -7, dtype=np.int32)))
    args = dict(E=E, N=N, pos_a=_p(d['a']), pos_b=_p(d['b']), natoms=_p(d['natoms']), select=_p(d['select']),
                aligned=_p(d['b']) if alias else None if no_aligned else _p(aligned.t), **{k: _p(out[k].t) for k in FIELDS})
    args.update(override(d) if callable(override) else override or {})
    rc = lib.mg_superpose(*[args[k] for k in ('E', 'N', 'pos_a', 'pos_b', 'natoms', 'select', 'aligned') + FIELDS], _stream())
    torch.cuda.synchronize()
    intact = all(o.intact() for o in out.values()) and (aligned is None or aligned.intact())
    got = {k: out[k].host() for k in FIELDS}
    got['rotation'] = got['rotation'].reshape(E, 3, 3)
    got['aligned'] = None if no_aligned else (d['b'] if alias else aligned.t).cpu().numpy()
    return rc, got, intact, d


def assert_row(got, e, w, b_row, n):
    for k in FIELDS:
        assert _same(got[k][e], getattr(w, k)), (e, k, got[k][e], getattr(w, k))
    if got['aligned'] is not None:
        assert _same(got['aligned'][e, :n], w.aligned), e
        assert got['aligned'][e, n:].tobytes() == b_row[n:].tobytes(), e  # slots beyond the atoms: B's bytes


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('name', list(EF_CASES))
def test_superpose_against_the_host_mirror(built_lib, name, masked):
    a, b, natoms, select, want = pairs(name)
    rc, got, intact, d = launch(built_lib, a, b, natoms, select if masked else None)
    assert rc == 0 and intact, built_lib.mg_last_error()
    for e, n in enumerate(natoms):
        w = want[masked][e]
        print(name, 'row', e, 'n', n, 'rmsd', got['rmsd'][e], 'displacement', got['displacement'][e], 'max deviation', got['max_deviation'][e])
        assert_row(got, e, w, b[e], n)
        assert w.ok and (w.rmsd > 0.0) == (n - (masked and n > e % 3) >= 2)
    assert _same(d['a'].cpu().numpy(), a) and _same(d['b'].cpu().numpy(), b) and _same(d['natoms'].cpu().numpy(), natoms)  # inputs are inputs
    assert not masked or _same(d['select'].cpu().numpy(), select)


@pytest.mark.parametrize('name', ['70', '255x1'])
def test_superpose_into_its_second_input_and_without_aligned(built_lib, name):
    a, b, natoms, select, want = pairs(name)
    rc, got, intact, d = launch(built_lib, a, b, natoms, select, alias=True)
    assert rc == 0 and intact
    for e, n in enumerate(natoms):
        assert_row(got, e, want[True][e], b[e], n)
    assert _same(d['a'].cpu().numpy(), a)
    rc, got, intact, d = launch(built_lib, a, b, natoms, select, no_aligned=True)
    assert rc == 0 and intact and _same(d['b'].cpu().numpy(), b)
    for e, n in enumerate(natoms):
        assert_row(got, e, want[True][e], b[e], n)


def test_rows_that_cannot_be_superposed(built_lib):
    """a NaN coordinate of a selected atom: NONFINITE by the mirror too; an atom count outside 0 .. N: NONFINITE and nothing of the
    row indexed; NaN outputs and B's bytes in `aligned` for the whole row; the rows between them come out as if alone"""
    a, b, natoms, _, _ = pairs('7')
    a, b, natoms = a.copy(), b.copy(), np.array([7, 7, 5, 6, 5], dtype=np.int32)
    a[:, :, :] = canvases(7, [7] * 5, seed=77)[0]
    for e in range(5):
        b[e] = moved(a[e], 0.05, seed=90 + e)
    b[2, 5:], a[2, 5:] = np.nan, np.nan
    b[1, 3, 1] = np.nan
    want = [S.superpose_host(a[e, :n], b[e, :n]) for e, n in enumerate(natoms)]
    natoms[2], natoms[3] = 8, -1
    rc, got, intact, _ = launch(built_lib, a, b, natoms)
    assert rc == 0 and intact
    for e in (0, 1, 4):
        assert_row(got, e, want[e], b[e], int(natoms[e]))
    assert [want[0].status, want[1].status, want[4].status] == [S.OK, S.NONFINITE, S.OK] and want[0].rmsd > 0.0 and want[4].rmsd > 0.0
    for e in (1, 2, 3):
        assert got['status'][e] == S.NONFINITE and got['aligned'][e].tobytes() == b[e].tobytes()
        assert all(np.isnan(got[k][e]).all() for k in FIELDS[:6])


def test_entry_point_refuses_bad_arguments(built_lib):
    a, b, natoms, select, _ = pairs('7')
    bad = [dict(E=0), dict(E=-1), dict(N=0), dict(N=256), dict(E=1 << 23, N=255), lambda d: dict(aligned=_p(d['a']))]
    bad += [{k: None} for k in ('pos_a', 'pos_b', 'natoms') + FIELDS]
    for override in bad:
        rc, got, intact, d = launch(built_lib, a, b, natoms, select, override=override)
        assert rc == -1 and intact, override
        # no kernel ran: the outputs hold what they held, the inputs too
        assert all((got[k] == (-7 if k == 'status' else -777.0)).all() for k in FIELDS + ('aligned', )), override
        assert _same(d['a'].cpu().numpy(), a) and _same(d['b'].cpu().numpy(), b)


# ---- superpose, superpose_canvases, and relax with superpose=True ---------------------------------------------------------------------
def _assert_superposed(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert all(_same(getattr(g, k), getattr(w, k)) for k in FIELDS) and g.ok == w.ok
        assert g.aligned.shape == w.aligned.shape and _same(g.aligned, w.aligned)


def test_superpose_of_lists_and_of_resident_tensors(built_lib):
    a, b, natoms, select, want = pairs('70')
    A, B = [a[e, :n] for e, n in enumerate(natoms)], [b[e, :n] for e, n in enumerate(natoms)]
    _assert_superposed(S.superpose(A, B), want[False])
    _assert_superposed(S.superpose(A, B, select=[select[e, :n].astype(bool) for e, n in enumerate(natoms)]), want[True])
    _assert_superposed(S.superpose(A[:2], B[:2], select=[0, 2, 5]), [S.superpose_host(x, y, select=[0, 2, 5]) for x, y in zip(A[:2], B[:2])])
    d = [torch.from_numpy(x).cuda() for x in (a, b, natoms, select)]
    got = S.superpose_canvases(d[0], d[1], d[2], select=d[3].bool())
    assert all(t.is_cuda for t in got.values()) and got['rotation'].shape == (5, 3, 3)
    for e, n in enumerate(natoms):
        row = {k: got[k].cpu().numpy() for k in FIELDS + ('aligned', )}
        assert_row(row, e, want[True][e], b[e], n)
    # in place: B itself takes the aligned positions
    work = d[1].clone()
    again = S.superpose_canvases(d[0], work, d[2], select=d[3], out=work)
    assert again['aligned'] is work and _same(work.cpu().numpy(), got['aligned'].cpu().numpy()) and torch.equal(again['rmsd'], got['rmsd'])


def _sampled():
    if 'sampled' not in _CACHE:
        from molgym_amd.episodes import sample_molecules
        _CACHE['sampled'] = sample_molecules(_agent(), FORMULAS, 8, num_envs=4, seed=3, min_atomic_distance=1.0)
    return _CACHE['sampled']


def test_relax_with_superpose_equals_relax_and_the_mirror(built_lib):
    R = PairReward(ZS4, A_EPS, A_SIGMA)
    mols = _sampled()
    plain, got = X.relax(R, mols), X.relax(R, mols, superpose=True)
    assert len(got) == len(plain) == len(mols)
    for m, p, g in zip(mols, plain, got):
        assert (g.status, g.iterations, g.evaluations) == (p.status, p.iterations, p.evaluations)
        assert _same(g.energy_before, p.energy_before) and _same(g.energy, p.energy) and _same(g.max_gradient, p.max_gradient)
        assert g.positions.tobytes() == p.positions.tobytes()
        assert (p.rmsd, p.displacement, p.max_deviation) == (None, None, None)
        w = S.superpose_host(m.positions, g.positions)
        print('n', len(m.numbers), 'iterations', g.iterations, 'rmsd', g.rmsd, 'displacement', g.displacement, 'max deviation', g.max_deviation)
        assert _same(g.rmsd, w.rmsd) and _same(g.displacement, w.displacement) and _same(g.max_deviation, w.max_deviation)
        assert g.rmsd <= g.displacement * (1 + 1e-12) + 1e-15
    assert any(g.rmsd > 0.0 for g in got)


def test_relax_canvases_with_superpose_on_a_resident_canvas(built_lib):
    from molgym_amd.episodes import DeviceEpisodes
    from tests.test_gpu_episodes_env import WATER
    R = PairReward(ZS4, A_EPS, A_SIGMA)
    start = tuple(WATER) + ((0, (0.0, 0.0, 0.0)), ) * 4
    eps = DeviceEpisodes(_agent(), FORMULAS, 6, initial=(start, (0, 4, 1, 0)), min_atomic_distance=1.0)
    eps.run(num_steps=3, seed=5)
    cv = eps.canvas
    before = cv.pos64.clone()
    plain = X.relax_canvases(R, cv.pos64, cv.charges, cv.natoms_dev, superpose=False)
    assert set(plain) == {'positions', 'energy_before', 'energy', 'max_gradient', 'iterations', 'evaluations', 'status'}
    got = X.relax_canvases(R, cv.pos64, cv.charges, cv.natoms_dev, superpose=True)
    assert set(got) == set(plain) | {'rmsd', 'displacement', 'max_deviation'} and all(t.is_cuda for t in got.values())
    assert all(torch.equal(got[k], plain[k]) for k in plain) and torch.equal(cv.pos64, before)
    want = S.superpose_canvases(cv.pos64, got['positions'], cv.natoms_dev)
    assert all(t.is_cuda for t in want.values())
    for k in ('rmsd', 'displacement', 'max_deviation'):
        assert _same(got[k].cpu().numpy(), want[k].cpu().numpy()), k
    print('rmsd', got['rmsd'].cpu().numpy(), 'displacement', got['displacement'].cpu().numpy())
    assert (want['status'] == S.OK).all() and (got['rmsd'] > 0).any()
    with pytest.raises(ValueError):
        X.relax_canvases(R, cv.pos64, cv.charges, cv.natoms_dev, out=cv.pos64, superpose=True)
