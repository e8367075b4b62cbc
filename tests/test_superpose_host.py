"""molgym_amd/structure.py on the host: the float64 mirror `superpose_host` against an SVD Kabsch written here, its exact
properties, the degenerate shapes, `select`, the rows that cannot be superposed, and the refusals of `superpose_host`,
`superpose`, `superpose_canvases` and of `relax`'s keyword, which come before anything touches a device.

The clusters are those of tests/test_gpu_relax.py::canvases: n sites of a lattice of spacing 1.12 with a normal jitter of sigma
0.05.  B = A jittered by `jitter`, turned by a random proper rotation and shifted."""
import numpy as np
import pytest

from molgym_amd import structure as S
from tests.test_gpu_relax import canvases

SIZES = [2, 3, 4, 7, 63, 64, 65, 255]
JITTERS = [0.0, 0.05, 0.5]
# 10 x the largest |superpose_host - Kabsch| over the 24 fixtures SIZES x JITTERS (profiles/superpose.md, "Against an SVD Kabsch":
# 2.38e-15 in the rmsd, 2.22e-15 in an entry of the rotation; other LAPACK builds round differently, hence the factor)
RMSD_BOUND = 2.38e-14
ROTATION_BOUND = 2.23e-14


def cluster(n, seed=0):
    return canvases(max(n, 1), [n], seed=1000 + n + seed)[0][0, :n].copy()


def moved(a, jitter, seed):
    """a jittered, turned by a random proper rotation (QR of a normal matrix, the determinant made +1) and shifted"""
    rng = np.random.RandomState(seed)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.linalg.det(q))
    noise = rng.normal(scale=jitter, size=a.shape) if jitter else 0.0
    return (a + noise) @ q.T + rng.normal(scale=2.0, size=3)


def kabsch(a, b):
    """(rmsd, rotation) of b laid on a: SVD of the covariance, the determinant corrected to a proper rotation"""
    a1, b1 = a - a.mean(axis=0), b - b.mean(axis=0)
    u, _, vt = np.linalg.svd(b1.T @ a1)
    d = np.sign(np.linalg.det(vt.T @ u.T))
    rot = vt.T @ np.diag([1.0, 1.0, d]) @ u.T
    res = a1 - b1 @ rot.T
    return np.sqrt((res * res).sum() / len(a)), rot


def test_mirror_against_an_svd_kabsch():
    worst_rmsd, worst_rot = 0.0, 0.0
    for n in SIZES:
        a = cluster(n)
        for jitter in JITTERS:
            b = moved(a, jitter, seed=n)
            got = S.superpose_host(a, b)
            rmsd, rot = kabsch(a, b)
            d_rmsd = abs(got.rmsd - rmsd)
            d_rot = np.abs(got.rotation - rot).max() if n >= 4 and jitter > 0 else 0.0
            print(f'n {n} jitter {jitter} rmsd {got.rmsd:.6e} |rmsd - kabsch| {d_rmsd:.2e} |rotation - kabsch| {d_rot:.2e} '
                  f'displacement {got.displacement:.4f} max deviation {got.max_deviation:.4e}')
            worst_rmsd, worst_rot = max(worst_rmsd, d_rmsd), max(worst_rot, d_rot)
            assert got.ok and got.displacement > 0.1 and got.rmsd <= got.max_deviation <= got.rmsd * np.sqrt(n) * (1 + 1e-12) + 1e-300
            assert got.rmsd < 1e-13 if jitter == 0.0 else (n < 4 or got.rmsd > 0.2 * jitter)
            # what the fields mean: aligned = rotation (b - centroid_b) + centroid_a, to rounding
            assert np.abs(got.aligned - ((b - got.centroid_b) @ got.rotation.T + got.centroid_a)).max() < 1e-12
    print('largest |rmsd - kabsch|', worst_rmsd, 'largest |rotation - kabsch|', worst_rot)
    assert worst_rmsd <= RMSD_BOUND and worst_rot <= ROTATION_BOUND


@pytest.mark.parametrize('n', [1, 3, 7, 65])
def test_a_structure_on_itself(n):
    """rmsd and max_deviation are 0.0 and the rotation has the identity's bytes: M is symmetric to the bit, so K01 = K02 = K03 are
    +0.0, the pairs (0, q) are skipped in every sweep, V[:, 0] stays (1, 0, 0, 0) and K00 = sum |a'|^2 is the largest diagonal
    entry.  `aligned` is (a - ca) + ca -- one rounding of a' + ca, where a' carries a rounding of its own -- to the last bit, which
    is within 2^-52 max(|a|, |ca|) of a, not always a itself."""
    a = cluster(n)
    got = S.superpose_host(a, a)
    assert got.ok and got.rmsd == 0.0 and got.max_deviation == 0.0 and got.displacement == 0.0
    assert got.rotation.tobytes() == np.eye(3).tobytes()
    assert got.centroid_a.tobytes() == got.centroid_b.tobytes()
    assert got.aligned.tobytes() == ((a - got.centroid_a) + got.centroid_a).tobytes()
    assert np.abs(got.aligned - a).max() <= 2.0**-52 * max(np.abs(a).max(), np.abs(got.centroid_a).max())


def test_a_mirror_image_is_not_superposed_by_a_reflection():
    a = cluster(7)
    b = a * np.array([-1.0, 1.0, 1.0])
    got = S.superpose_host(a, b)
    rmsd, rot = kabsch(a, b)
    print('rmsd of the mirror image', got.rmsd, 'kabsch', rmsd, 'det - 1', np.linalg.det(got.rotation) - 1.0)
    assert got.ok and got.rmsd > 0.1 and abs(np.linalg.det(got.rotation) - 1.0) <= 1e-12
    assert abs(got.rmsd - rmsd) <= RMSD_BOUND and np.linalg.det(rot) > 0.0


def _degenerate():
    rng = np.random.RandomState(5)
    line = np.outer(np.arange(5) * 1.12 + rng.normal(scale=0.05, size=5), [0.48, -0.6, 0.64])
    plane = cluster(6)
    plane = plane - np.outer(plane @ np.array([0.6, 0.0, 0.8]), [0.6, 0.0, 0.8])
    return {'one atom': cluster(1), 'two atoms': cluster(2), 'five collinear': line, 'six coplanar': plane}


@pytest.mark.parametrize('jitter', [0.0, 0.05])
@pytest.mark.parametrize('shape', ['one atom', 'two atoms', 'five collinear', 'six coplanar'])
def test_degenerate_shapes(shape, jitter):
    a = _degenerate()[shape]
    b = moved(a, jitter, seed=len(a))
    got = S.superpose_host(a, b)
    rmsd, _ = kabsch(a, b)
    print(shape, 'jitter', jitter, 'rmsd', got.rmsd, 'kabsch', rmsd, 'difference', abs(got.rmsd - rmsd))
    assert got.ok and abs(got.rmsd - rmsd) <= RMSD_BOUND and abs(np.linalg.det(got.rotation) - 1.0) <= 1e-12
    if shape == 'one atom':
        assert got.rmsd == 0.0 and got.max_deviation == 0.0 and got.displacement > 0.0


def _same_fit(x, y):
    return (x.rmsd == y.rmsd and x.displacement == y.displacement and x.max_deviation == y.max_deviation and x.status == y.status
            and x.rotation.tobytes() == y.rotation.tobytes() and x.centroid_a.tobytes() == y.centroid_a.tobytes()
            and x.centroid_b.tobytes() == y.centroid_b.tobytes())


def _selected_case():
    a = cluster(65)
    b = moved(a, 0.05, seed=3)
    mask = np.arange(65) % 3 != 1
    b[~mask] += 0.7  # the unselected atoms lie elsewhere: they must not enter the fit
    return a, b, mask


def test_select_takes_the_fit_from_the_selected_atoms_and_transforms_all():
    """the fit does not see the unselected atoms -- other coordinates there, a NaN among them, give the same bits -- a mask and
    an index list are one thing, and `aligned` holds every atom"""
    a, b, mask = _selected_case()
    got = S.superpose_host(a, b, select=mask)
    a2, b2 = a.copy(), b.copy()
    a2[~mask], b2[~mask] = -3.0, 11.0
    b2[1, 2] = np.nan
    assert _same_fit(got, S.superpose_host(a2, b2, select=mask)) and _same_fit(got, S.superpose_host(a, b, select=np.flatnonzero(mask)))
    rb = (b - got.centroid_b) @ got.rotation.T + got.centroid_a
    assert got.aligned.shape == (65, 3) and np.abs(got.aligned - rb).max() < 1e-12 and np.linalg.norm(got.aligned[~mask] - a[~mask], axis=1).min() > 0.5
    assert not _same_fit(got, S.superpose_host(a, b))
    alone = S.superpose_host(a[mask], b[mask])
    assert abs(got.rmsd - alone.rmsd) <= RMSD_BOUND and np.abs(got.rotation - alone.rotation).max() <= ROTATION_BOUND


def test_select_of_the_leading_atoms_is_the_subset_alone():
    a, b, _ = _selected_case()
    for m in (1, 2, 7, 64):
        got, alone = S.superpose_host(a, b, select=np.arange(65) < m), S.superpose_host(a[:m], b[:m])
        assert _same_fit(got, alone) and got.aligned[:m].tobytes() == alone.aligned.tobytes()


def test_select_of_scattered_atoms_is_the_subset_alone_bit_for_bit():
    """the k-th selected atom sits in slot k of every sum, where it sits when the subset is given alone: rmsd, displacement,
    max_deviation, rotation and centroids have the same bits, and so has `aligned` of the selected atoms"""
    a, b, mask = _selected_case()
    got, alone = S.superpose_host(a, b, select=mask), S.superpose_host(a[mask], b[mask])
    print('rmsd', abs(got.rmsd - alone.rmsd), 'rotation', np.abs(got.rotation - alone.rotation).max(), 'centroids',
          max(np.abs(got.centroid_a - alone.centroid_a).max(), np.abs(got.centroid_b - alone.centroid_b).max()))
    assert _same_fit(got, alone) and got.aligned[mask].tobytes() == alone.aligned.tobytes()
    for n, keep in ((7, [6, 0, 3]), (255, list(range(1, 255, 2))), (70, [64]), (65, [0, 64])):
        a, sel = cluster(n), np.zeros(n, dtype=bool)
        b = moved(a, 0.05, seed=n)
        sel[keep] = True
        assert _same_fit(S.superpose_host(a, b, select=keep), S.superpose_host(a[sel], b[sel])), n


def test_no_selected_atom():
    a, b = cluster(4), moved(cluster(4), 0.05, seed=1)
    for x, y, sel in ((a, b, np.zeros(4, dtype=bool)), (a, b, []), (a[:0], b[:0], None), ([], [], None)):
        got = S.superpose_host(x, y, select=sel)
        assert got.ok and (got.rmsd, got.displacement, got.max_deviation) == (0.0, 0.0, 0.0)
        assert got.rotation.tobytes() == np.eye(3).tobytes() and not got.centroid_a.any() and not got.centroid_b.any()
        assert got.aligned.tobytes() == np.asarray(y, dtype=np.float64).tobytes() and got.aligned.shape == (len(x), 3)


@pytest.mark.parametrize('bad', [np.nan, np.inf, -np.inf, 1e200])
@pytest.mark.parametrize('side', ['a', 'b'])
def test_a_coordinate_that_is_not_finite(bad, side):
    """in a selected atom: NONFINITE, NaN outputs, aligned = B's bytes (1e200: D overflows); in an unselected atom: OK, the bits that
    finite coordinates there give"""
    a = cluster(7)
    b = moved(a, 0.05, seed=2)
    (a if side == 'a' else b)[4, 1] = bad
    got = S.superpose_host(a, b)
    assert got.status == S.NONFINITE and not got.ok and np.isnan([got.rmsd, got.displacement, got.max_deviation]).all()
    assert np.isnan(got.rotation).all() and np.isnan(got.centroid_a).all() and np.isnan(got.centroid_b).all()
    assert got.aligned.tobytes() == b.tobytes()
    mask = np.arange(7) != 4
    off = S.superpose_host(a, b, select=mask)
    clean_a, clean_b = a.copy(), b.copy()
    clean_a[4], clean_b[4] = 0.0, 0.0
    assert off.ok and _same_fit(off, S.superpose_host(clean_a, clean_b, select=mask)) and np.isfinite(off.aligned[mask]).all()
    assert np.isfinite(off.aligned[4]).all() == (side == 'a' or bad == 1e200)


def test_bad_arguments_are_value_errors():
    a = cluster(4)
    for x, y, kw in ((a, a[:3], {}), (a.reshape(-1), a, {}), (a[:, :2], a[:, :2], {}), (np.zeros((256, 3)), np.zeros((256, 3)), {}),
                     (a, a, dict(select=np.ones(3, dtype=bool))), (a, a, dict(select=[4])), (a, a, dict(select=[-1])),
                     (a, a, dict(select=[0.5]))):
        with pytest.raises(ValueError):
            S.superpose_host(x, y, **kw)
    # `superpose`: refused before anything touches a device
    for A, B, kw in (([a], [a, a], {}), ([a], [a[:3]], {}), ([np.zeros((256, 3))], [np.zeros((256, 3))], {}), ([a, a], [a, a], dict(select=[[0], [1], [2]])),
                     ([a], [a], dict(select=[7])), ([a, a[:2]], [a, a[:2]], dict(select=np.ones(4, dtype=bool)))):
        with pytest.raises(ValueError):
            S.superpose(A, B, **kw)
    assert S.superpose([], []) == []


def test_superpose_canvases_refuses_bad_tensors():
    import torch
    E, N = 2, 4
    good = dict(pos_a=torch.zeros(E, N, 3, dtype=torch.float64), pos_b=torch.zeros(E, N, 3, dtype=torch.float64),
                natoms_dev=torch.zeros(E, dtype=torch.int32))
    pa = good['pos_a']
    bad = [dict(pos_a=pa.float()), dict(pos_b=pa.float()), dict(pos_a=pa[:, :, :2]), dict(pos_a=pa[0]), dict(pos_b=pa[:1]),
           dict(pos_a=pa.transpose(0, 1)), dict(natoms_dev=good['natoms_dev'].long()), dict(natoms_dev=torch.zeros(3, dtype=torch.int32)),
           dict(select=torch.zeros(E, N)), dict(select=torch.zeros(E, N + 1, dtype=torch.bool)), dict(out=pa), dict(out=pa.float()),
           dict(out=torch.zeros(E, N + 1, 3, dtype=torch.float64)), dict(pos_a=torch.zeros(E, 256, 3, dtype=torch.float64), pos_b=torch.zeros(E, 256, 3, dtype=torch.float64)),
           dict(pos_a=torch.zeros(0, N, 3, dtype=torch.float64), pos_b=torch.zeros(0, N, 3, dtype=torch.float64), natoms_dev=torch.zeros(0, dtype=torch.int32)),
           dict(pos_b=torch.zeros(E, N, 3, dtype=torch.float64, device='meta'))]
    for override in bad:
        with pytest.raises(ValueError):
            S.superpose_canvases(**{**good, **override})


def test_relax_refuses_a_superpose_that_is_not_a_bool():
    from molgym_amd import relax as X
    from molgym_amd.rewards import PairReward
    R = PairReward([0, 1, 6], [0.0, 0.8, 1.0], [0.0, 0.95, 1.0])
    for value in (1, 0, None, 'yes'):
        with pytest.raises(ValueError):
            X.relax(R, [([1, 1], np.zeros((2, 3)))], superpose=value)
    done = X.relax_host(R, [1, 6], [[0.0, 0.0, 0.0], [1.1, 0.0, 0.0]])
    assert (done.rmsd, done.displacement, done.max_deviation) == (None, None, None)


def test_the_package_exports_the_names_lazily():
    import molgym_amd
    assert molgym_amd.superpose is S.superpose and molgym_amd.superpose_host is S.superpose_host
    assert molgym_amd.superpose_canvases is S.superpose_canvases and molgym_amd.Superposed is S.Superposed
