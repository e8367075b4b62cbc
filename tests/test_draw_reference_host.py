"""tests/draw_ref.py on the CPU (the role tests/test_gemm_reference_host.py has for tests/gemm_ref.py): the mirror of the keyed
random numbers against known answers and as a generator, the float32 restatements of the draw kernels against the float64
replays on every input family of tests/test_gpu_draws.py (inside the ambiguity caps), the recorded tolerances against their
measurement, and planted defects, each of which the replay must reject."""
import functools

import numpy as np
import pytest

from tests import draw_ref as D

SEED = 0x5EED1234ABCD
HALF_W, CENTER = float(np.float32(0.5)), float(np.float32(1.3))       # distances in (0.8, 1.8)
INT_HALF = np.array([0.5, 0.5 * np.pi, 0.5 * np.pi], dtype=np.float32)
INT_CEN = np.array([1.3, 0.5 * np.pi, 0.5 * np.pi], dtype=np.float32)


# ---- the generator --------------------------------------------------------------------------------------------------------
def test_splitmix64_known_answers():
    """the published first outputs of the seed-0 sequence (state advances by the golden gamma before each output)"""
    gamma = 0x9E3779B97F4A7C15
    want = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    got = [int(D.splitmix64((k * gamma) & (2**64 - 1))[0]) for k in range(3)]
    assert got == want


def test_u01_range_and_the_closed_top_end(monkeypatch):
    u = D.u01(SEED, np.arange(1 << 10)[:, None], 1, np.arange(1 << 10)[None, :])
    assert u.dtype == np.float32 and u.min() > 0 and u.max() <= 1
    assert 7e-8 < u.min() < 1e-5 and 0.99999 < u.max()
    assert abs(u.mean() - 0.5) < 5 / np.sqrt(12 * u.size)
    # h >> 40 = 2^24 - 1: (float)(2^24 - 1) + 0.5f rounds to 2^24, the value is exactly 1.0 -- the interval is (0, 1]
    monkeypatch.setattr(D, 'splitmix64', lambda x: np.full(np.atleast_1d(x).shape, 2**64 - 1, dtype=np.uint64))
    assert D.u01(0, 0, 0, 0).item() == 1.0
    monkeypatch.setattr(D, 'splitmix64', lambda x: np.zeros(np.atleast_1d(x).shape, dtype=np.uint64))
    assert D.u01(0, 0, 0, 0).item() == np.float32(0.5) * np.float32(2.0**-24)


def test_u01_is_uniform_and_uncorrelated_across_its_axes():
    n = 1 << 20
    u = D.u01(SEED, np.arange(n), 2, 0).astype(np.float64)
    chi2 = ((np.bincount((u * 64).astype(int).clip(0, 63), minlength=64) - n / 64)**2 / (n / 64)).sum()
    assert chi2 < 63 + 5 * np.sqrt(126)
    m = 1 << 16
    base = D.u01(SEED, np.arange(m), 2, 5).astype(np.float64)
    for other in (D.u01(SEED, np.arange(m) + 1, 2, 5), D.u01(SEED, np.arange(m), 3, 5), D.u01(SEED, np.arange(m), 2, 6),
                  D.u01(SEED + 1, np.arange(m), 2, 5)):
        assert abs(np.corrcoef(base, other.astype(np.float64))[0, 1]) < 5 / np.sqrt(m)


@pytest.mark.parametrize('keys', [D.cov_keys(), D.int_keys()])
def test_no_two_sub_actions_share_a_key(keys):
    """the inner key is (stream << 24) ^ draw: one stream per sub-action and every draw below 2^24 keep them apart"""
    streams = [s for s, _ in keys.values()]
    assert len(set(streams)) == len(streams) and max(streams) < 256
    assert max(n for _, n in keys.values()) - 1 <= 3 * 8192 * 256 + 2 < 2**24
    lo = D.u01(SEED, 7, [s for s, _ in keys.values()], 0)
    hi = D.u01(SEED, 7, [s for s, _ in keys.values()], [n - 1 for _, n in keys.values()])
    assert len(set(lo.tolist())) == len(streams) and np.all(hi > 0)


# ---- input families: the shapes and scales of tests/test_gpu_draws.py -------------------------------------------------------
def _cat_family(name, rng):
    """(logits f32 [R][L], valid [R][L], kernel loop length [R])"""
    kind, L, scale = name
    R = 512
    z = (scale * rng.normal(size=(R, L))).astype(np.float32)
    if kind == 'focus':          # the real atoms first; an empty canvas is one entry of logit 0
        n = rng.integers(0, L + 1, size=R)
        n[:4] = (0, 1, min(64, L), L)
        valid = np.arange(L)[None, :] < np.maximum(n, 1)[:, None]
        z[n == 0, 0] = 0.0
        return z, valid, np.maximum(n, 1)
    if kind == 'element':        # bags: random, one element left, first / last / alternating symbols zeroed
        valid = rng.integers(0, 2, size=(R, L)).astype(bool)
        valid[:, 0] = False
        q = R // 4
        valid[:q] = False
        valid[np.arange(q), rng.integers(1, L, size=q)] = True
        valid[q:q + 8, :L // 2], valid[q:q + 8, L // 2:] = False, True
        valid[q + 8:q + 16, :L // 2], valid[q + 8:q + 16, L // 2:] = True, False
        valid[q + 8:q + 16, 0] = False
        valid[q + 16:q + 24] = (np.arange(L) % 2 == 1)[None, :]
        valid[~valid.any(axis=1), 1] = True
        return z, valid, np.full(R, L)
    return z, np.ones((R, L), dtype=bool), np.full(R, L)   # 'plain': kappa (2), the mixture component (G)


CAT_FAMILIES = [('focus', 7, 1.0), ('focus', 7, 30.0), ('focus', 7, 0.0), ('focus', 20, 1.0), ('focus', 255, 1.0),
                ('focus', 255, 30.0), ('focus', 255, 0.0), ('element', 3, 1.0), ('element', 3, 30.0), ('element', 3, 0.0),
                ('element', 9, 1.0), ('element', 16, 1.0), ('element', 16, 30.0), ('plain', 2, 1.0), ('plain', 8, 1.0)]


@pytest.mark.parametrize('family', CAT_FAMILIES, ids=lambda f: f'{f[0]}{f[1]}x{f[2]:g}')
@pytest.mark.parametrize('mode', [D.TRAIN, D.EVAL])
def test_honest_float32_categorical_passes(family, mode):
    rng = np.random.default_rng(CAT_FAMILIES.index(family))
    z, valid, length = _cat_family(family, rng)
    u = D.u01(SEED, D.samples_of(3, 5, len(z)), 0, 0)
    want, amb = D.categorical(z, valid, u, mode, length)
    got = D.honest_f32_categorical(z, valid, u, mode)
    share, rows = D.check(got, want, amb, D.CAP_CATEGORICAL, str(family))
    assert rows >= 0.95 * len(z)
    assert np.all(valid[np.arange(len(z)), want])


def _gmm_inputs(G, rng, R=256):
    o = rng.normal(size=(R, 2 * G)).astype(np.float32)
    logstd = (np.log(0.1) + 0.2 * rng.normal(size=G)).astype(np.float32)
    return o, logstd


def _so3_inputs(rng, R, peaked=False):
    coef = rng.normal(size=(R, 25, 4, 2)).astype(np.float32)
    coef *= (0.5**np.repeat(np.arange(5), 2 * np.arange(5) + 1))[None, :, None, None].astype(np.float32)  # smoother fields
    empty = np.zeros(R, dtype=bool)
    empty[:2] = True
    coef[:2] = 0.0            # an empty canvas conditions on nothing
    coef[2:5, 1:] = 0.0       # one atom: a constant density, every candidate ranks the same
    return coef, empty


@pytest.mark.parametrize('G', [1, 3, 8])
def test_honest_float32_gmm_passes(G):
    rng = np.random.default_rng(G)
    o, logstd = _gmm_inputs(G, rng)
    s = D.samples_of(3, 5, len(o))
    u = [D.u01(SEED, s, 2, j) for j in range(3)]
    want, amb = D.gmm(o, logstd, G, HALF_W, CENTER, *u)
    D.check(D.honest_f32_gmm(o, logstd, G, HALF_W, CENTER, *u), want, amb, D.CAP_CATEGORICAL, f'gmm G={G}')
    o, logstd = o[:48], logstd
    want, amb = D.gmm_best_of(o, logstd, G, HALF_W, CENTER, SEED, s[:48])
    D.check(D.honest_f32_gmm_best_of(o, logstd, G, HALF_W, CENTER, SEED, s[:48]), want, amb, D.CAP_BEST_OF, f'gmm best-of G={G}')


@pytest.mark.parametrize('mode', [D.TRAIN, D.EVAL])
def test_honest_float32_normal3_passes(mode):
    rng = np.random.default_rng(11)
    cout = rng.normal(size=(256, 3)).astype(np.float32)
    cout[:8, 0] = -6.0        # means at the lower edge: with a wide sigma the clamp acts
    logstd = np.array([np.log(0.9), np.log(0.2), np.log(0.3)], dtype=np.float32)
    u = D.normal3_uniforms(SEED, D.samples_of(0, 1, 256))
    want, amb = D.normal3(cout, logstd, INT_HALF, INT_CEN, u, mode)
    assert mode == D.EVAL or (want[:, 0] == 0.001).sum() > 0
    D.check(D.honest_f32_normal3(cout, logstd, INT_HALF, INT_CEN, u, mode), want, amb, 0.0, 'normal3')


SO3_CASES = [(1, 1.0, D.TRAIN, 70), (0, None, D.TRAIN, 70), (1, 1.0, D.EVAL, 24), (0, None, D.EVAL, 24)]


@functools.lru_cache(maxsize=None)
def _so3_run(case):
    has_beta, beta, mode, R = case
    coef, empty = _so3_inputs(np.random.default_rng(17), R)
    s = D.samples_of(3, 5, R)
    t64, t32 = [], []
    want, amb = D.so3_reject(coef, has_beta, beta, empty, SEED, s, mode, trace=t64)
    got = D.honest_f32_so3(coef, has_beta, beta, empty, SEED, s, mode, trace=t32)
    return coef, empty, s, want, amb, got, t64, t32


@pytest.mark.parametrize('case', SO3_CASES, ids=lambda c: f'beta{c[1]}-mode{c[2]}')
def test_honest_float32_orientation_passes(case):
    coef, empty, s, want, amb, got, t64, _ = _so3_run(case)
    cap = D.CAP_SO3_TRAIN if case[2] == D.TRAIN else D.CAP_BEST_OF
    D.check(got, want, amb, cap, f'so3 {case}')
    assert np.abs(np.linalg.norm(want, axis=1) - 1).max() < 1e-12
    scanned = np.array([len(t[0]) for t in t64])
    assert scanned.max() < 256 * 64    # (the acceptance rate of these coefficients: far from the 8192-round limit)


INT_LOGSTD = np.log(np.array([0.15, 0.25, 0.25])).astype(np.float32)     # SchNetAC's initial widths


@functools.lru_cache(maxsize=None)
def _measured():
    """worst deviation of the float32 restatements from the float64 replays over the families above:
    (continuous values and direction components, gap between the two best ranking values of a best-of draw,
    acceptance probability)"""
    value, acc, gap = 0.0, 0.0, 0.0
    for G in (1, 3, 8):
        rng = np.random.default_rng(G)
        o, logstd = _gmm_inputs(G, rng)
        s = D.samples_of(3, 5, len(o))
        u = [D.u01(SEED, s, 2, j) for j in range(3)]
        want, amb = D.gmm(o, logstd, G, HALF_W, CENTER, *u)
        got = D.honest_f32_gmm(o, logstd, G, HALF_W, CENTER, *u)
        value = max(value, np.abs(got - want)[~amb].max())
        lps = []
        D.honest_f32_gmm_best_of(o, logstd, G, HALF_W, CENTER, SEED, s, lp_out=lps)
        c32, lp32 = np.stack([c for c, _ in lps], axis=1), np.stack([lp for _, lp in lps], axis=1).astype(np.float64)
        lp64 = D.gmm_logp(o, logstd, G, HALF_W, CENTER, c32.astype(np.float64))
        top2 = np.argsort(lp64, axis=1)[:, -2:]
        g32, g64 = (np.take_along_axis(v, top2, axis=1) for v in (lp32, lp64))
        gap = max(gap, np.abs((g32[:, 1] - g32[:, 0]) - (g64[:, 1] - g64[:, 0])).max())
    rng = np.random.default_rng(11)
    cout = rng.normal(size=(256, 3)).astype(np.float32)
    u = D.normal3_uniforms(SEED, D.samples_of(0, 1, 256))
    value = max(value, np.abs(D.honest_f32_normal3(cout, INT_LOGSTD, INT_HALF, INT_CEN, u, D.TRAIN) -
                              D.normal3(cout, INT_LOGSTD, INT_HALF, INT_CEN, u, D.TRAIN)[0]).max())
    for case in SO3_CASES:
        _, _, _, want, amb, got, t64, t32 = _so3_run(case)
        value = max(value, np.abs(got - want)[~amb].max())
        for (p64, v64, a64), (p32, v32, a32), a in zip(t64, t32, amb):
            n = min(len(p64), len(p32)) if a else len(p64)
            assert a or (len(p64) == len(p32) and np.array_equal(a64, a32))
            acc = max(acc, np.abs(p64[:n] - p32[:n]).max())
            if case[2] == D.EVAL and not a:
                top2 = np.nonzero(a64)[0][np.argsort(v64[a64])[-2:]]
                gap = max(gap, abs((v32[top2[1]] - v32[top2[0]]) - (v64[top2[1]] - v64[top2[0]])))
    return value, gap, acc


def test_recorded_tolerances_are_eight_times_the_measured_deviation():
    """VALUE_TOL, RANK_TOL and DELTA_ACC of draw_ref.py: measured here (float32 restatement against float64 replay, same
    inputs), never on a device; the recorded figure is 8x the measurement, rounded up"""
    value, gap, acc = _measured()
    print(f'measured: value {value:.4e} (VALUE_TOL {D.VALUE_TOL:.3e}), gap of the two best {gap:.4e} (RANK_TOL {D.RANK_TOL:.3e}), '
          f'acceptance {acc:.4e} (DELTA_ACC {D.DELTA_ACC:.3e})')
    assert 8 * value <= D.VALUE_TOL <= 8.5 * value
    assert 8 * gap <= D.RANK_TOL <= 8.5 * gap
    assert 8 * acc <= D.DELTA_ACC <= 8.5 * acc


# ---- planted defects: each must be rejected -------------------------------------------------------------------------------------
def _rejected(fn):
    with pytest.raises(AssertionError, match='differ from the replay'):
        fn()


def test_planted_categorical_defects_are_rejected():
    rng = np.random.default_rng(5)
    z, valid, length = _cat_family(('element', 16, 1.0), rng)
    s = D.samples_of(3, 5, len(z))
    u = D.u01(SEED, s, 1, 0)
    want, amb = D.categorical(z, valid, u, D.TRAIN, length)
    D.check(D.honest_f32_categorical(z, valid, u, D.TRAIN), want, amb, D.CAP_CATEGORICAL, 'honest')
    for defect in ('shifted', 'masked_counted'):
        _rejected(lambda: D.check(D.honest_f32_categorical(z, valid, u, D.TRAIN, defect=defect), want, amb, D.CAP_CATEGORICAL, defect))
    # the stream ids of focus (0) and element (1) exchanged; the stride of the sample ids ignored
    _rejected(lambda: D.check(D.honest_f32_categorical(z, valid, D.u01(SEED, s, 0, 0), D.TRAIN), want, amb, D.CAP_CATEGORICAL, 'streams'))
    _rejected(lambda: D.check(D.honest_f32_categorical(z, valid, D.u01(SEED, D.samples_of(3, 1, len(z)), 1, 0), D.TRAIN), want, amb,
                              D.CAP_CATEGORICAL, 'stride'))
    # one single row off by one among 512 is enough
    got = D.honest_f32_categorical(z, valid, u, D.TRAIN)
    row = int(np.nonzero(~amb & (valid.sum(axis=1) > 1))[0][0])
    got[row] = np.nonzero(valid[row] & (np.arange(16) != got[row]))[0][0]
    _rejected(lambda: D.check(got, want, amb, D.CAP_CATEGORICAL, 'one row'))


def test_planted_continuous_defects_are_rejected():
    rng = np.random.default_rng(6)
    o, logstd = _gmm_inputs(3, rng)
    o[:16, 3:] = -6.0                              # means at 0.8 ...
    wide = np.full(3, np.log(0.9), dtype=np.float32)  # ... under a sigma of 0.9: the clamp acts on some rows
    s = D.samples_of(0, 1, len(o))
    u = [D.u01(SEED, s, 2, j) for j in range(3)]
    want, amb = D.gmm(o, wide, 3, HALF_W, CENTER, *u)
    assert (want == 0.001).sum() > 0
    D.check(D.honest_f32_gmm(o, wide, 3, HALF_W, CENTER, *u), want, amb, D.CAP_CATEGORICAL, 'honest')
    for defect in ('sin_for_cos', 'no_clamp'):
        _rejected(lambda: D.check(D.honest_f32_gmm(o, wide, 3, HALF_W, CENTER, *u, defect=defect), want, amb, D.CAP_CATEGORICAL, defect))
    cout = rng.normal(size=(256, 3)).astype(np.float32)
    cout[:16, 0] = -6.0
    un = D.normal3_uniforms(SEED, s)
    want, amb = D.normal3(cout, wide, INT_HALF, INT_CEN, un, D.TRAIN)
    assert (want[:, 0] == 0.001).sum() > 0
    for defect in ('sin_for_cos', 'no_clamp'):
        _rejected(lambda: D.check(D.honest_f32_normal3(cout, wide, INT_HALF, INT_CEN, un, D.TRAIN, defect=defect), want, amb, 0.0, defect))
    # evaluation best-of count halved (64 candidates where the kernel takes 128)
    want, amb = D.gmm_best_of(o[:48], logstd, 3, HALF_W, CENTER, SEED, s[:48])
    _rejected(lambda: D.check(D.honest_f32_gmm_best_of(o[:48], logstd, 3, HALF_W, CENTER, SEED, s[:48], count=64), want, amb,
                              D.CAP_BEST_OF, 'best-of halved'))


@pytest.mark.parametrize('case,defect', [(SO3_CASES[0], 'best_in_training'), (SO3_CASES[1], 'best_in_training'),
                                         (SO3_CASES[0], 'half_envelope'), (SO3_CASES[1], 'half_envelope'),
                                         (SO3_CASES[2], 'best_of_halved'), (SO3_CASES[3], 'best_of_halved')])
def test_planted_orientation_defects_are_rejected(case, defect):
    coef, empty, s, want, amb, _, _, _ = _so3_run(case)
    has_beta, beta, mode, R = case
    got = D.honest_f32_so3(coef, has_beta, beta, empty, SEED, s, mode, defect=defect)
    cap = D.CAP_SO3_TRAIN if mode == D.TRAIN else D.CAP_BEST_OF
    _rejected(lambda: D.check(got, want, amb, cap, defect))
