"""The host statement of the hull rule, the refill cycle and the formula draw (tests/episode_rules_ref.py) against the
reference's own statements (environment.py:143-249), and the refusals of `DeviceEpisodes`' rule keywords.  No GPU."""
import types

import numpy as np
import pytest

from molgym_amd import episodes
from tests import episode_rules_ref as X

ZS = [0, 1, 6, 8]


# ---- hull -------------------------------------------------------------------------------------------------------------------
def _scaffolds():
    tetra = np.array([(2.0, 2.0, 2.0), (2.0, -2.0, -2.0), (-2.0, 2.0, -2.0), (-2.0, -2.0, 2.0)])
    octa = 2.5 * np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], dtype=np.float64)
    return [(tetra, 4), (octa, 8), (X.fibonacci_sphere(34, 3.0), 64), (X.fibonacci_sphere(35, 3.0), 66)]


@pytest.mark.parametrize('which', [0, 1, 2, 3])
def test_half_spaces_equal_find_simplex(which):
    """environment.py:167-171 on 20 000 points; a point within 1e-9 of a facet may fall either way and is left out"""
    pts, num_planes = _scaffolds()[which]
    planes = X.hull_planes(pts)
    assert planes.shape == (num_planes, 4)
    assert np.allclose(np.linalg.norm(planes[:, :3], axis=1), 1.0, atol=1e-12)  # unit normals: hull_tol is a distance
    q = np.random.RandomState(0).uniform(-3.5, 3.5, size=(20000, 3))
    m = X.hull_max(planes, q)
    keep = np.abs(m) > 1e-9
    assert np.mean(~keep) <= 0.001
    got, want = X.inside_hull(planes, q)[keep], X.inside_scaffold_reference(pts, q)[keep]
    print(f'scaffold {which}: {int((~keep).sum())} left out, {int((got != want).sum())} disagreements, inside share {got.mean():.3f}')
    assert np.array_equal(got, want)
    assert 0.02 < got.mean() < 0.5  # both answers occur
    # one point at a time, as the rules call it
    for i in range(5):
        assert bool(X.inside_hull(planes, q[i])) == bool(m[i] <= 0.0)


def test_hull_tol_moves_the_faces_outward():
    planes = X.hull_planes(_scaffolds()[1][0])
    q = np.array([2.5 + 0.05, 0.0, 0.0])  # beyond the +x vertex of the octahedron
    d = float(X.hull_max(planes, q))
    assert d > 0 and not X.inside_hull(planes, q) and X.inside_hull(planes, q, hull_tol=d) and not X.inside_hull(planes, q, np.nextafter(d, 0))


# ---- formula draw -----------------------------------------------------------------------------------------------------------
COUNTS, LO, HI, SEED, DRAWS = (0, 4, 1, 1), 2, 7, 20240607, 100000  # C1 H4 O1


def _within(k, n, p, what):
    sd = np.sqrt(n * p * (1 - p))
    assert abs(k - n * p) <= 4 * sd, f'{what}: {k} of {n}, expected {n * p:.1f} +- {sd:.1f}'


def test_integer_draws_have_the_reference_distribution():
    """environment.py:240-249: sizes uniform on [lo, hi), symbols with probability count / size; validity as the closed form"""
    bags, valid, sizes = X.formula_tries(COUNTS, ZS, LO, HI, SEED, np.arange(DRAWS), 0)
    assert np.array_equal(bags.sum(axis=1), sizes) and sizes.min() == LO and sizes.max() == HI - 1
    for s in range(LO, HI):
        _within(int((sizes == s).sum()), DRAWS, 1.0 / (HI - LO), f'size {s}')
    total = int(sizes.sum())
    for i, c in enumerate(COUNTS):
        if c == 0:
            assert bags[:, i].sum() == 0
        else:
            _within(int(bags[:, i].sum()), total, c / sum(COUNTS), f'symbol {i}')
    parity = (bags * np.array([0, 1, 4, 2])).sum(axis=1) % 2
    assert np.array_equal(valid, parity == 0)
    _within(int(valid.sum()), DRAWS, episodes.formula_validity(COUNTS, ZS, (LO, HI)), 'valid first tries')
    # a fixed size: lo == hi draws hi symbols (environment.py:243-244)
    bags, valid, sizes = X.formula_tries(COUNTS, ZS, 5, 5, SEED, np.arange(DRAWS), 0)
    assert np.all(sizes == 5) and np.all(bags.sum(axis=1) == 5)
    _within(int(valid.sum()), DRAWS, episodes.formula_validity(COUNTS, ZS, (5, 5)), 'valid first tries, size 5')
    assert episodes.formula_validity(COUNTS, ZS, (5, 5)) == pytest.approx((1 + (1 - 2 * 4 / 6)**5) / 2)


def test_accepted_formulas_have_even_bond_parity_and_match_the_tries():
    first = X.formula_tries(COUNTS, ZS, LO, HI, SEED, np.arange(300), 0)
    later = 0
    for b in range(300):
        bag = X.draw_formula(COUNTS, ZS, LO, HI, 64, SEED, b)
        assert bag is not None and sum(int(c) * X.BOND_COUNT[z] for c, z in zip(bag, ZS) if c) % 2 == 0
        if first[1][b]:
            assert np.array_equal(bag, first[0][b])
        else:
            later += 1
            assert np.array_equal(bag, next(x for x, ok in (X.formula_try(COUNTS, ZS, LO, HI, SEED, b, t) for t in range(1, 64)) if ok))
    assert 0 < later < 300
    assert X.draw_formula((0, 1, 0, 0), ZS, 3, 3, 64, SEED, 0) is None  # three H: never valid, and the loop ends
    # the 24 bits are the ones rng_u01 turns into its float
    from tests import draw_ref as D
    r = X.u24(SEED, np.arange(50), 4, 7)
    assert np.array_equal(D.u01(SEED, np.arange(50), 4, 7), ((r.astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)))


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def _stub(zs, canvas_size):
    """an agent without a device: the rule keywords are checked before the device is"""
    return types.SimpleNamespace(zs=list(zs), theta=types.SimpleNamespace(device=types.SimpleNamespace(type='cpu')),
                                 observation_space=types.SimpleNamespace(canvas_space=types.SimpleNamespace(size=canvas_size)))


def _scaffold_obs(points, zs, label, canvas_size, bag):
    canvas = tuple((label, tuple(float(x) for x in p)) for p in points)
    return canvas + ((0, (0.0, 0.0, 0.0)), ) * (canvas_size - len(points)), tuple(bag)


def test_rule_keywords_are_refused_without_a_device():
    ac = _stub(ZS, 6)
    with pytest.raises(ValueError, match='probability'):
        episodes.DeviceEpisodes(ac, [((1, 1), )], 4, size_range=(3, 3))  # H only, a fixed odd size: never valid
    with pytest.raises(ValueError, match='bond count'):
        episodes.DeviceEpisodes(_stub([0, 1, 16], 6), [((16, 1), (1, 2))], 4, size_range=(2, 5))
    with pytest.raises(ValueError, match='refills'):
        episodes.DeviceEpisodes(ac, [((6, 1), (1, 4), (8, 1))], 4, size_range=(2, 5), num_refills=1)
    with pytest.raises(ValueError, match='one formula'):
        episodes.DeviceEpisodes(ac, [((6, 1), (1, 4)), ((8, 1), (1, 2))], 4, size_range=(2, 5))
    with pytest.raises(ValueError):
        episodes.DeviceEpisodes(ac, [((6, 1), (1, 4), (8, 1))], 4, size_range=(5, 2))
    with pytest.raises(ValueError):
        episodes.DeviceEpisodes(ac, [((6, 1), (1, 4), (8, 1))], 4, size_range=(2, 5), max_formula_tries=65)
    zs5 = [0, 1, 6, 8, 16]
    ac5 = _stub(zs5, 10)
    octa = 2.5 * np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], dtype=np.float64)
    good = _scaffold_obs(octa, zs5, 4, 10, (0, 2, 0, 1, 0))
    with pytest.raises(ValueError, match='scaffold element'):
        episodes.DeviceEpisodes(ac5, [((1, 2), (16, 1))], 4, initial=good, scaffold_z=16)
    flat = _scaffold_obs(octa[:4], zs5, 4, 10, (0, 2, 0, 1, 0))  # four atoms in the plane z = 0
    with pytest.raises(ValueError, match='coplanar'):
        episodes.DeviceEpisodes(ac5, [((1, 2), (8, 1))], 4, initial=flat, scaffold_z=16)
    with pytest.raises(ValueError, match='at least 4'):
        episodes.DeviceEpisodes(ac5, [((1, 2), (8, 1))], 4, initial=_scaffold_obs(octa[:3], zs5, 4, 10, (0, 2, 0, 1, 0)), scaffold_z=16)
    with pytest.raises(ValueError, match='ONE initial'):
        episodes.DeviceEpisodes(ac5, [((1, 2), (8, 1))], 4, initial=[good] * 4, scaffold_z=16)
    with pytest.raises(ValueError, match='not among zs'):
        episodes.DeviceEpisodes(ac5, [((1, 2), (8, 1))], 4, initial=good, scaffold_z=7)
    with pytest.raises(ValueError):
        episodes.DeviceEpisodes(ac5, [((1, 2), (8, 1))], 4, num_refills=-1)
    # configurations that pass every check reach the device test instead
    for kw in (dict(initial=good, scaffold_z=16), dict(num_refills=2)):
        with pytest.raises(RuntimeError, match='HIP device only'):
            episodes.DeviceEpisodes(ac5, [((1, 2), (8, 1))], 4, **kw)
    with pytest.raises(RuntimeError, match='HIP device only'):
        episodes.DeviceEpisodes(ac, [((6, 1), (1, 4), (8, 1))], 4, size_range=(2, 5))
    assert len(episodes.STATUS_NAMES) == 10 and episodes.STATUS_NAMES[X.REFILLED] == 'REFILLED' and episodes.STATUS_NAMES[X.OUTSIDE] == 'OUTSIDE'
    assert X.REFILLED in episodes.ATOM_STATUSES and X.OUTSIDE in episodes.DONE_STATUSES and X.REFILLED not in episodes.DONE_STATUSES
    ep = episodes.Episode(0, 0, np.zeros(0), np.zeros((0, 3)), X.STOP, np.zeros(1), np.zeros(1))
    assert ep.refills == 0 and ep.bag == ()


# ---- refill cycle -----------------------------------------------------------------------------------------------------------
def test_refill_cycle_worked_by_hand():
    """environment.py:190-207 with F = 2, num_refills = 1: reset takes formula 0, the refill formula 1, the second emptying ends
    the episode; the next reset goes on in the SAME cycle: 0, 1 | 0, 1.  With three formulas the cycle does not realign:
    0, 1 | 2, 0 | 1, 2."""
    C1, O1, H1 = (0, 0, 1, 0), (0, 0, 0, 1), (0, 1, 0, 0)
    for formulas, want in (([C1, O1], [(0, 1), (0, 1), (0, 1)]), ([C1, O1, H1], [(0, 1), (2, 0), (1, 2)])):
        env = X.RulesEnvX(8, ZS, formulas, 0.5, 2.0, num_refills=1)
        seen = []
        for _ in want:
            first = env.formula_no % len(formulas)
            assert env.refills == 0 and env.bag == list(formulas[first])
            _, _, done, info = env.step((formulas[first].index(1), (0.0, 0.0, 0.0)))
            assert info['status'] == X.REFILLED and not done and env.refills == 1
            second = env.formula_no % len(formulas)
            assert env.bag == list(formulas[second])
            _, _, done, info = env.step((formulas[second].index(1), (1.0, 0.0, 0.0)))
            assert info['status'] == X.BAG_EMPTY and done  # no refill left
            assert env.given == [a + b for a, b in zip(formulas[first], formulas[second])]
            seen.append((first, second))
            env.reset()
        assert seen == want


def test_full_canvas_consumes_no_refill_and_the_array_model_agrees():
    """environment.py:191-192; and `episode_step_rules` (the model of the kernel's arrays) walks the same cycle as the class"""
    C1, O1 = (0, 0, 1, 0), (0, 0, 0, 1)
    env = X.RulesEnvX(1, ZS, [C1, O1], 0.5, 2.0, num_refills=1)
    _, _, done, info = env.step((2, (0.0, 0.0, 0.0)))
    assert info['status'] == X.FULL and done and env.refills == 0 and env.formula_no == 0
    N, E = 3, 1
    st = dict(pos64=np.zeros((E, N, 3)), pos32=np.zeros((E, N, 3), dtype=np.float32), charges=np.zeros((E, N), dtype=np.int32),
              bags=np.array([C1], dtype=np.float32), natoms=np.zeros(E, dtype=np.int32), alive=np.ones(E, dtype=np.int32),
              episode_no=np.zeros(E, dtype=np.int32), start_pos64=np.zeros((E, N, 3)), start_charges=np.zeros((E, N), dtype=np.int32),
              start_natoms=np.zeros(E, dtype=np.int32), formulas=np.array([C1, O1], dtype=np.float32),
              refills=np.zeros(E, dtype=np.int32), formula_no=np.zeros(E, dtype=np.int32))
    env = X.RulesEnvX(N, ZS, [C1, O1], 0.5, 2.0, num_refills=1)
    trace = []
    for t, (el, x) in enumerate([(2, 0.0), (3, 1.0), (2, 0.0), (3, 1.0), (2, 0.0)]):
        acts = np.zeros((E, 7), dtype=np.float32)
        acts[0, 2] = el
        status, _ = X.episode_step_rules(st, ZS, acts, np.array([[x, 0.0, 0.0]]), 0.5, 2.0, False, num_refills=1)
        _, _, done, info = env.step((el, (x, 0.0, 0.0)))
        if done:
            env.reset()
        assert status[0] == info['status']
        assert (int(st['formula_no'][0]), int(st['refills'][0]), int(st['episode_no'][0])) == (env.formula_no, env.refills, env.episode)
        assert list(st['bags'][0]) == env.bag and int(st['natoms'][0]) == len(env.atoms)
        trace.append(int(status[0]))
    assert trace == [X.REFILLED, X.BAG_EMPTY, X.REFILLED, X.BAG_EMPTY, X.REFILLED]
