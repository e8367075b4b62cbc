"""PairReward (molgym_amd/rewards.py) on the host: the float64 mirror against an independent evaluation of the Lennard-Jones
formula, the mixing tables, the edge cases of the order contract, and every refusal.  No GPU."""
import math
import types

import numpy as np
import pytest

from molgym_amd import _lib, rollout
from molgym_amd.rewards import PairReward

ZS = [0, 1, 6, 8]
EPS = [0.0, 0.031, 0.105, 0.152]
SIGMA = [0.0, 1.1, 1.7, 1.52]


def _independent(R, numbers, positions, new_z, q):
    """4 eps ((sigma / r)^12 - (sigma / r)^6), summed by math.fsum in Python floats, minus the penalty"""
    a = R.zs.index(new_z)
    terms = []
    for z, p in zip(numbers, positions):
        b = R.zs.index(int(z))
        r = math.sqrt(sum((float(x) - float(y))**2 for x, y in zip(q, p)))
        if R.cutoff is not None and r > R.cutoff:
            continue
        eps, sigma = math.sqrt(EPS[a] * EPS[b]), (SIGMA[a] + SIGMA[b]) / 2
        terms.append(4 * eps * ((sigma / r)**12 - (sigma / r)**6))
    return -(math.fsum(terms) + R.distance_penalty * math.sqrt(sum(float(x)**2 for x in q)))


def _molecule(rng, n):
    """n atoms at least 0.9 apart, numbers from ZS[1:]"""
    pts = []
    while len(pts) < n:
        c = rng.uniform(-2.5, 2.5, size=3)
        if all(np.linalg.norm(c - p) > 0.9 for p in pts):
            pts.append(c)
    return rng.choice(ZS[1:], size=n), np.array(pts).reshape(-1, 3)


@pytest.mark.parametrize('cutoff', [None, 2.6])
def test_host_mirror_against_an_independent_evaluation(cutoff):
    R = PairReward(ZS, EPS, SIGMA, distance_penalty=0.07, cutoff=cutoff)
    rng = np.random.RandomState(3)
    before, new_z, new_pos = [], [], []
    for n in (1, 2, 5, 17, 40):
        numbers, positions = _molecule(rng, n + 1)
        before.append((numbers[:n], positions[:n]))
        new_z.append(int(numbers[n]))
        new_pos.append(positions[n])
    got = R.host(before, np.array(new_z), np.array(new_pos), np.arange(len(before)))
    assert got.dtype == np.float64 and got.shape == (5, )
    for k, (numbers, positions) in enumerate(before):
        want = _independent(R, numbers, positions, new_z[k], new_pos[k])
        assert abs(got[k] - want) <= 1e-12 * abs(want), (k, got[k], want)
    if cutoff is not None:  # the cutoff matters in these molecules, and does not zero everything
        free = PairReward(ZS, EPS, SIGMA, distance_penalty=0.07).host(before, np.array(new_z), np.array(new_pos), np.arange(5))
        assert (got != free).any() and (got[2:] != -0.07 * np.linalg.norm(np.array(new_pos), axis=1)[2:]).all()


def test_mixing_tables():
    R = PairReward(ZS, EPS, SIGMA)
    Z = len(ZS)
    for t in (R.four_eps, R.sigma2):
        assert t.dtype == np.float64 and t.shape == (Z, Z) and t.flags['C_CONTIGUOUS'] and np.array_equal(t, t.T)
    for i in range(Z):
        for j in range(Z):
            sig = (np.float64(SIGMA[i]) + np.float64(SIGMA[j])) / 2.0
            assert R.sigma2[i, j] == sig * sig and R.four_eps[i, j] == 4.0 * np.sqrt(np.float64(EPS[i]) * np.float64(EPS[j]))
    # full tables are taken as they are
    eps = np.array([[0.1, 0.2, 0.3], [0.2, 0.4, 0.5], [0.3, 0.5, 0.6]])
    sig = np.array([[1.0, 1.1, 1.2], [1.1, 1.3, 1.4], [1.2, 1.4, 1.5]])
    T = PairReward([0, 1, 8], eps, sig)
    assert np.array_equal(T.four_eps, 4.0 * eps) and np.array_equal(T.sigma2, sig * sig)
    # per-element epsilon with a full sigma table
    M = PairReward([0, 1, 8], [0.1, 0.4, 0.6], sig)
    assert np.array_equal(M.sigma2, sig * sig) and M.four_eps[1, 2] == 4.0 * np.sqrt(np.float64(0.4) * np.float64(0.6))


def test_no_atoms_coincident_atoms_and_the_fold_order():
    R = PairReward(ZS, EPS, SIGMA, distance_penalty=0.25)
    q = np.array([0.3, -0.4, 1.2])
    none = (np.zeros(0, dtype=np.int64), np.zeros((0, 3)))
    got = R.host([none], np.array([6]), q[None], np.array([0]))
    assert got[0] == -(np.float64(0.25) * np.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]))
    # a coincident atom: inf - inf = NaN, which pays -inf -- wherever it sits in the row
    numbers, positions = np.array([1, 8, 6]), np.array([[0.0, 0.0, 0.0], [0.3, -0.4, 1.2], [1.5, 0.0, 0.0]])
    assert R.host([(numbers, positions)], np.array([6]), q[None], np.array([0]))[0] == float('-inf')
    assert R.host([(numbers[1:2], positions[1:2])], np.array([1]), q[None], np.array([0]))[0] == float('-inf')
    # sequential in slot order: the fold of the terms one by one, not np.sum's pairwise tree
    rng = np.random.RandomState(0)
    numbers, positions = _molecule(rng, 41)
    a = R.zs.index(int(numbers[40]))
    qq = positions[40]
    terms = []
    for z, p in zip(numbers[:40], positions[:40]):
        d = qq - p
        terms.append(R.pair(a, R.zs.index(int(z)), (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
    dE = terms[0]
    for V in terms[1:]:
        dE = dE + V
    want = -(dE + np.float64(0.25) * np.sqrt((qq[0] * qq[0] + qq[1] * qq[1]) + qq[2] * qq[2]))
    assert R.host([(numbers[:40], positions[:40])], numbers[40:41], qq[None], np.array([0]))[0] == want


def test_cutoff_zeroes_exactly_the_pairs_beyond_it():
    cutoff = 2.0
    R, free = PairReward(ZS, EPS, SIGMA, cutoff=cutoff), PairReward(ZS, EPS, SIGMA)
    q = np.zeros(3)
    # r2 == cutoff^2 exactly (kept), one ulp above (dropped), well inside, well outside
    above = np.nextafter(2.0, 3.0)
    positions = np.array([[2.0, 0.0, 0.0], [0.0, above, 0.0], [0.0, 0.0, 1.3], [3.0, 0.0, 0.0]])
    numbers = np.array([6, 6, 8, 1])
    assert above * above > cutoff * cutoff
    each = [free.host([(numbers[j:j + 1], positions[j:j + 1])], np.array([6]), q[None], np.array([0]))[0] for j in range(4)]
    cut = [R.host([(numbers[j:j + 1], positions[j:j + 1])], np.array([6]), q[None], np.array([0]))[0] for j in range(4)]
    assert all(v != 0.0 for v in each)
    assert cut[0] == each[0] and cut[2] == each[2] and cut[1] == 0.0 and cut[3] == 0.0
    # and in one row: the kept terms alone, in their order
    V0 = free.pair(2, 2, np.float64(4.0))
    V2 = free.pair(2, 3, np.float64(1.3) * np.float64(1.3))
    assert R.host([(numbers, positions)], np.array([6]), q[None], np.array([0]))[0] == -(((V0 + 0.0) + V2) + 0.0)


def test_refusals():
    with pytest.raises(ValueError, match='negative or non-finite'):
        PairReward(ZS, [0.0, -0.1, 0.1, 0.1], SIGMA)
    with pytest.raises(ValueError, match='negative or non-finite'):
        PairReward(ZS, EPS, [0.0, 1.0, float('nan'), 1.0])
    with pytest.raises(ValueError, match='negative or non-finite'):
        PairReward(ZS, [0.0, float('inf'), 0.1, 0.1], SIGMA)
    asym = np.array([[1.0, 1.1, 1.2], [1.1, 1.3, 1.4], [1.25, 1.4, 1.5]])
    with pytest.raises(ValueError, match='not symmetric'):
        PairReward([0, 1, 8], [0.1, 0.2, 0.3], asym)
    with pytest.raises(ValueError, match='not symmetric'):
        PairReward([0, 1, 8], asym, [1.0, 1.0, 1.0])
    with pytest.raises(ValueError, match='len\\(zs\\)'):
        PairReward([1], [0.1], [1.0])
    many = list(range(_lib.MG_MAX_Z + 1))
    with pytest.raises(ValueError, match='len\\(zs\\)'):
        PairReward(many, [0.1] * len(many), [1.0] * len(many))
    PairReward(many[:-1], [0.1] * _lib.MG_MAX_Z, [1.0] * _lib.MG_MAX_Z)  # MG_MAX_Z itself is allowed
    with pytest.raises(ValueError, match='shape'):
        PairReward(ZS, EPS[:3], SIGMA)
    for bad in (0.0, -1.0, float('nan')):
        with pytest.raises(ValueError, match='cutoff'):
            PairReward(ZS, EPS, SIGMA, cutoff=bad)
    for bad in (-0.1, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='distance_penalty'):
            PairReward(ZS, EPS, SIGMA, distance_penalty=bad)


def _stub(zs, canvas_size):
    return types.SimpleNamespace(zs=list(zs), theta=types.SimpleNamespace(device=types.SimpleNamespace(type='cpu')),
                                 observation_space=types.SimpleNamespace(canvas_space=types.SimpleNamespace(size=canvas_size)))


def test_rollout_refusals_without_a_device():
    ac = _stub(ZS, 6)
    formulas = [((6, 1), (1, 4), (8, 1))]
    R = PairReward(ZS, EPS, SIGMA)
    with pytest.raises(ValueError, match='reward together with reward_fn'):
        rollout.DeviceRollout(ac, formulas, 4, 8, reward=R, reward_fn=R.host)
    with pytest.raises(ValueError, match='reward together with size_range'):
        rollout.DeviceRollout(ac, formulas, 4, 8, reward=R, size_range=(2, 5))
    with pytest.raises(ValueError, match='was built for zs'):
        rollout.DeviceRollout(ac, formulas, 4, 8, reward=PairReward([0, 1, 8, 6], EPS, SIGMA))
    with pytest.raises(ValueError, match='was built for zs'):
        rollout.DeviceRollout(ac, formulas, 4, 8, reward=PairReward([0, 1, 6], EPS[:3], SIGMA[:3]))
    # what passes these checks reaches DeviceEpisodes' own
    with pytest.raises(RuntimeError, match='HIP device only'):
        rollout.DeviceRollout(ac, formulas, 4, 8, reward=R)
