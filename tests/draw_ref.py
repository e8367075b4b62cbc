"""Host mirror of the keyed random numbers of csrc/sampling.inc and float64 replays of every rollout draw of both agents
(numpy + scipy only; nothing of molgym_amd is imported, same role as tests/gemm_ref.py for the GEMM kernels).

The device draws are deterministic functions of (i) the distribution parameters, which the workspace still holds after the
call, and (ii) uniforms u01(seed, base + stride * b, stream, draw) that the host recomputes bit for bit.  A replay returns
the action the device must have taken and, per row, an `ambiguous` flag: the row's uniform lies so close to a decision
boundary that float32 rounding on the device may legitimately decide the other way.  `check` demands equality on every other
row and bounds the ambiguous share.

Margins
  * categorical pick: delta(len) = (len + 8) * 2^-23 around every interior CDF boundary.  Derived: the kernel forms S and the
    running sum with `len` float32 additions each, every one rounding by at most 2^-24 of a partial sum <= 1 (together
    2 * len * 2^-24 = len * 2^-23); the p_i = expf(.) / S terms carry a few ulps each of a value <= 1 (the 8 * 2^-23).
  * arg-max of the evaluation mode: the two largest probabilities closer than 2^-20 relative -- unless the two logits are the
    SAME float32 number: equal inputs give equal expf on any device, and both sides then keep the first.
  * DELTA_ACC (acceptance probability of the orientation sampler), VALUE_TOL (continuous draws, directions per component) and
    RANK_TOL (the gap between the two best ranking values of a best-of draw: mixture log-density, orientation density) cannot
    be derived, they are MEASURED on the CPU: the worst deviation of the float32 restatements of the kernel arithmetic
    (`honest_f32_*` below) from the float64 replays over the input families of tests/test_draw_reference_host.py (the shapes
    and scales of tests/test_gpu_draws.py), times 8 because the device's expf / logf / cosf / tanhf are another libm than
    numpy's.  Nothing here comes from device output.

        quantity                                         measured (float32 vs float64)   used (x 8, rounded up)
        continuous draws, direction components           3.31e-7  (a direction component) VALUE_TOL = 2.7e-6
        gap between the two best ranking values          3.18e-7                          RANK_TOL  = 2.6e-6
        acceptance probability of the orientation draw   8.33e-7  (f / max f, no beta)    DELTA_ACC = 6.7e-6

    tests/test_draw_reference_host.py::test_recorded_tolerances_are_eight_times_the_measured_deviation re-measures them and
    fails when a recorded figure is below 8x, or above 8.5x, its measurement.  (The gap, not each value: the two best
    candidates of a row share every parameter, and most of a log-density's float32 error is common to both.  A best of 128
    normal draws has its two best log-densities within 2.6e-6 of each other in about 6 % of rows, whatever the widths.)
  * best-of draws: the two best ranking values closer than RANK_TOL -- unless every candidate is ranked by the same float32
    number (orientation coefficients of l >= 1 all exactly zero: the density of an empty or one-atom canvas is constant), where
    both sides keep the first accepted candidate.
  * one float32 quantisation is part of the replay, not of the margin: the azimuth of the Fibonacci grid point i,
    2 pi i / golden, reaches 1.6e4 rad where a float32 holds 1e-3 rad.  The envelope is the maximum over the grid the kernel
    actually evaluates, so the replay rounds that product and quotient to float32 (IEEE operations, the same on any device) and
    evaluates everything else in float64.
"""
import numpy as np

TRAIN, EVAL = 1, 2          # SAMPLE_TRAIN / SAMPLE_EVAL of sampling.inc
VALUE_TOL = 2.7e-6
RANK_TOL = 2.6e-6
DELTA_ACC = 6.7e-6
CAP_CATEGORICAL, CAP_SO3_TRAIN, CAP_BEST_OF = 0.05, 0.02, 0.10
SO3_MAX_ROUNDS = 8192       # k_sample_so3: rounds of 256 candidates
F32 = np.float32
_U64 = np.uint64


# ---- the keyed random numbers ---------------------------------------------------------------------------------------------
def splitmix64(x):
    """one round of the splitmix64 output function on (state + golden gamma), uint64 arithmetic with wrap-around"""
    x = np.atleast_1d(np.asarray(x, dtype=_U64)).copy()
    with np.errstate(over='ignore'):
        x += _U64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> _U64(27))) * _U64(0x94D049BB133111EB)
    return x ^ (x >> _U64(31))


def u01(seed, sample, stream, draw):
    """rng_u01 of sampling.inc for broadcastable integer arrays: float32 in (0, 1]"""
    sample = np.asarray(sample, dtype=np.int64).astype(np.uint32).astype(_U64)   # (uint32_t)(base + stride * b)
    stream = np.asarray(stream, dtype=_U64)
    draw = np.asarray(draw, dtype=_U64)
    sample, stream, draw = np.broadcast_arrays(sample, stream, draw)
    shape = sample.shape
    key = (sample.ravel() << _U64(32)) | ((stream.ravel() << _U64(24)) ^ draw.ravel())
    h = splitmix64(_U64(int(seed) & 0xFFFFFFFFFFFFFFFF) ^ splitmix64(key))
    u = ((h >> _U64(40)).astype(F32) + F32(0.5)) * F32(1.0 / 16777216.0)
    assert u.dtype == F32 and np.all(u > 0) and np.all(u <= 1)
    return u.reshape(shape)


def samples_of(base, stride, rows):
    """the stream ids of rows 0 .. rows-1 of a launch keyed (base, stride)"""
    return int(base) + int(stride) * np.arange(rows, dtype=np.int64)


# sub-action -> (stream, number of draws 0 .. n-1 it may read) of one step
def cov_keys():
    return {'focus': (0, 1), 'element': (1, 1), 'distance': (2, 3 + 3 * 128), 'orientation': (3, 3 * SO3_MAX_ROUNDS * 256)}


def int_keys():
    return {'focus': (0, 1), 'element': (1, 1), 'continuous': (2, 6), 'kappa': (3, 1)}


# ---- float64 replays ------------------------------------------------------------------------------------------------------
def delta(length):
    return (np.asarray(length, dtype=np.float64) + 8.0) * 2.0**-23


def _masked_probs(logits, valid):
    z = np.where(valid, np.asarray(logits, dtype=np.float64), -np.inf)
    any_valid = valid.any(axis=1)
    m = np.where(any_valid, z.max(axis=1, initial=-np.inf), 0.0)
    e = np.where(valid, np.exp(np.where(valid, z - m[:, None], 0.0)), 0.0)
    s = e.sum(axis=1)
    return e / np.where(s > 0, s, 1.0)[:, None], any_valid


def categorical(logits, valid, u, mode, length=None):
    """categorical_pick_at / is_cat_pick: logits [R][L] (float32 values), valid [R][L] bool, u [R].  `length`: the kernel's
    loop length per row (default L).  Returns (pick [R], ambiguous [R]).  A row without a valid entry picks 0."""
    logits = np.asarray(logits)
    valid = np.asarray(valid, dtype=bool)
    R, L = logits.shape
    u = np.asarray(u, dtype=np.float64)
    length = np.full(R, L) if length is None else np.asarray(length)
    p, any_valid = _masked_probs(logits, valid)
    idx = np.arange(L)[None, :]
    if mode == EVAL:
        pick = np.argmax(np.where(valid, p, -1.0), axis=1)
        top = p[np.arange(R), pick]
        same = logits == logits[np.arange(R), pick][:, None]       # bit-identical logits tie on every device alike
        rival = np.where(valid & ~same, p, -1.0).max(axis=1, initial=-1.0)
        amb = any_valid & (rival >= 0) & (top - rival < 2.0**-20 * top)
        return np.where(any_valid, pick, 0), amb
    cdf = np.cumsum(p, axis=1)
    last = np.where(any_valid, L - 1 - np.argmax(valid[:, ::-1], axis=1), 0)
    hit = valid & (u[:, None] < cdf)
    pick = np.where(hit.any(axis=1), np.argmax(hit, axis=1), last)
    interior = valid & (idx < last[:, None])
    amb = (interior & (np.abs(u[:, None] - cdf) < delta(length)[:, None])).any(axis=1)
    return pick, amb


def gmm_logp(o, logstd, G, half_w, center, x):
    """log-density of the mixture (gmm_logp of sampling.inc) in float64; o [R][2G], x [R] or [R][K]"""
    o = np.asarray(o, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    xs = x.reshape(x.shape[0], -1)[:, :, None]                                   # [R][K][1]
    w = o[:, :G]
    mx = w.max(axis=1, keepdims=True)
    lw = (w - (mx + np.log(np.exp(w - mx).sum(axis=1, keepdims=True))))[:, None, :]
    mean = (np.tanh(o[:, G:]) * float(half_w) + float(center))[:, None, :]
    sd = np.maximum(np.exp(np.asarray(logstd, dtype=np.float64)), 1e-6)[None, None, :]
    t = -(xs - mean)**2 / (2 * sd**2) - np.log(sd) - 0.9189385332046727 + lw
    tm = t.max(axis=-1, keepdims=True)
    return (tm + np.log(np.exp(t - tm).sum(axis=-1, keepdims=True)))[..., 0].reshape(x.shape)


def _gmm_draw(o, logstd, G, half_w, center, u0, u1, u2):
    o = np.asarray(o, dtype=np.float64)
    R = o.shape[0]
    g, amb = categorical(o[:, :G], np.ones((R, G), dtype=bool), u0, TRAIN)
    u1, u2 = np.asarray(u1, dtype=np.float64), np.asarray(u2, dtype=np.float64)
    sd = np.maximum(np.exp(np.asarray(logstd, dtype=np.float64)), 1e-6)[g]
    zn = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    return np.tanh(o[np.arange(R), G + g]) * float(half_w) + float(center) + sd * zn, amb


def gmm(o, logstd, G, half_w, center, u0, u1, u2):
    """k_sample_gmm, training mode: component by the categorical walk, Box-Muller, the 0.001 clamp"""
    x, amb = _gmm_draw(o, logstd, G, half_w, center, u0, u1, u2)
    return np.maximum(x, 0.001), amb


def gmm_best_of(o, logstd, G, half_w, center, seed, samples, count=128):
    """k_sample_gmm, evaluation mode: the best of `count` candidates (draws 3k+3 .. 3k+5 of stream 2) by the mixture
    log-density, the first one on ties; no clamp"""
    o = np.asarray(o, dtype=np.float64)
    R = o.shape[0]
    k = np.arange(count)[None, :]
    s = np.asarray(samples)[:, None]
    us = [u01(seed, s, 2, 3 * k + 3 + j) for j in range(3)]
    cand = np.empty((R, count))
    amb = np.zeros(R, dtype=bool)
    for c in range(count):
        cand[:, c], a = _gmm_draw(o, logstd, G, half_w, center, us[0][:, c], us[1][:, c], us[2][:, c])
        amb |= a
    lp = gmm_logp(o, logstd, G, half_w, center, cand)
    best = np.argmax(lp, axis=1)
    srt = np.sort(lp, axis=1)
    amb |= (srt[:, -1] - srt[:, -2] < RANK_TOL) if count > 1 else False
    return cand[np.arange(R), best], amb


def normal3(cout, logstd, half_w, center, u, mode):
    """k_int_draw_cont_place: distance / angle / dihedral of SchNetAC.  cout [R][3], u [R][3][2] (draws 2k, 2k+1 of stream
    2), half_w / center [3].  Evaluation mode returns the means.  Never ambiguous."""
    cout = np.asarray(cout, dtype=np.float64)
    mean = np.tanh(cout) * np.asarray(half_w, dtype=np.float64)[None, :] + np.asarray(center, dtype=np.float64)[None, :]
    amb = np.zeros(cout.shape[0], dtype=bool)
    if mode == EVAL:
        return mean, amb
    u = np.asarray(u, dtype=np.float64)
    zn = np.sqrt(-2.0 * np.log(u[:, :, 0])) * np.cos(2.0 * np.pi * u[:, :, 1])
    x = mean + np.exp(1e-6 + np.asarray(logstd, dtype=np.float64))[None, :] * zn
    x[:, 0] = np.maximum(x[:, 0], 0.001)
    return x, amb


def normal3_uniforms(seed, samples):
    s = np.asarray(samples)[:, None, None]
    return u01(seed, s, 2, 2 * np.arange(3)[None, :, None] + np.arange(2)[None, None, :])


_LM = [(l, m) for l in range(5) for m in range(-l, l + 1)]     # q = l*l + l + m


def ylm64(theta, phi):
    """[n][25] complex Y_lm (Condon-Shortley) of polar / azimuth angles, the convention tests/test_gpu_dists.py pins"""
    from scipy.special import sph_harm_y
    theta, phi = np.asarray(theta, dtype=np.float64), np.asarray(phi, dtype=np.float64)
    return np.stack([sph_harm_y(l, m, theta, phi) for l, m in _LM], axis=1)


_GRID = {}


def _grid_ylm(ngrid):
    """Y_lm on the Fibonacci grid of k_sample_so3: ct exact in float32 for a power-of-two grid, the azimuth rounded to float32
    as the kernel's (6.2831855f * (float)i) / 1.618034f is (see the module docstring)"""
    if ngrid not in _GRID:
        i = np.arange(ngrid, dtype=F32)
        ct = F32(1) - F32(2) * (i + F32(0.5)) / F32(ngrid)
        ph = (F32(6.283185307179586) * i) / F32(1.618033988749895)
        assert ct.dtype == F32 and ph.dtype == F32
        _GRID[ngrid] = ylm64(np.arccos(ct.astype(np.float64)), ph.astype(np.float64))
    return _GRID[ngrid]


def so3_reject(coef, has_beta, beta, empty, seed, samples, mode, chunk=None, trace=None):
    """k_sample_so3.  coef [R][25][CE][2] (float32 values of the conditioned coefficients), empty [R] bool (canvas without
    atoms), samples [R] stream ids.  Returns (direction [R][3], ambiguous [R]).  `trace` (a list) receives per row the
    acceptance probabilities, ranking values and acceptance flags of the candidates scanned, for the tolerance measurement."""
    coef = np.asarray(coef, dtype=np.float64)
    R = coef.shape[0]
    a = coef.sum(axis=2)
    a = a[:, :, 0] + 1j * a[:, :, 1]                                   # [R][25]
    k = np.maximum((np.abs(a)**2).sum(axis=1), 1e-10)
    ngrid = 4096 if has_beta else 1024
    fg = np.abs(_grid_ylm(ngrid) @ a.T)**2 / k[None, :]                # [ngrid][R]
    vmax = ((-beta * fg) if has_beta else fg).max(axis=0)
    need = 1 if mode == TRAIN else (128 if has_beta else 256)
    chunk = chunk or (32 if mode == TRAIN else 512)
    out = np.tile(np.array([0.0, 0.0, 1.0]), (R, 1))
    amb = np.zeros(R, dtype=bool)
    for r in range(R):
        accept_all = bool(empty[r]) and not has_beta
        have, best, start = 0, -np.inf, 0
        second = -np.inf
        tr_p, tr_v, tr_a = [], [], []
        while have < need and start < SO3_MAX_ROUNDS * 256:
            i = np.arange(start, min(start + chunk, SO3_MAX_ROUNDS * 256))
            u1, u2, u3 = (u01(seed, samples[r], 3, 3 * i + j).astype(np.float64) for j in range(3))
            ct = 1.0 - 2.0 * u1
            st = np.sqrt(np.maximum(0.0, 1.0 - ct * ct))
            ph = 2.0 * np.pi * u2
            f = np.abs(ylm64(np.arccos(ct), ph) @ a[r])**2 / k[r]
            val = -beta * f if has_beta else f
            p = np.ones_like(f) if accept_all else (np.exp(val - vmax[r]) if has_beta else f / vmax[r])
            acc = np.ones_like(f, dtype=bool) if accept_all else (u3 < p)
            near = np.zeros_like(acc) if accept_all else (np.abs(u3 - p) < DELTA_ACC)
            order = np.nonzero(acc)[0]
            stop = len(i) if have + len(order) < need else int(order[need - have - 1]) + 1   # candidates scanned
            amb[r] |= bool(near[:stop].any())
            tr_p.append(p[:stop]); tr_v.append(val[:stop]); tr_a.append(acc[:stop])
            for c in order[order < stop]:
                have += 1
                if mode == TRAIN or val[c] > best:
                    second = max(second, best)
                    best = val[c]
                    out[r] = (st[c] * np.cos(ph[c]), st[c] * np.sin(ph[c]), ct[c])
                else:
                    second = max(second, val[c])
            start += len(i)
        # (coefficients of l >= 1 that are all exactly zero -- an empty or one-atom canvas -- rank every candidate by the SAME
        # float32 number on any device: both sides keep the first accepted one, as with bit-identical logits)
        if mode == EVAL and best - second < RANK_TOL and np.any(coef[r, 1:]):
            amb[r] = True
        if trace is not None:
            trace.append((np.concatenate(tr_p), np.concatenate(tr_v), np.concatenate(tr_a)))
    return out, amb


# ---- the comparison -------------------------------------------------------------------------------------------------------
def check(got, want, ambiguous, cap, what=''):
    """every non-ambiguous row must match (integer picks exactly, floating values within VALUE_TOL per component); the
    ambiguous share must stay <= cap.  Returns (ambiguous share, rows compared)."""
    got, want = np.asarray(got), np.asarray(want)
    ambiguous = np.asarray(ambiguous, dtype=bool)
    assert got.shape == want.shape and ambiguous.shape == got.shape[:1], (what, got.shape, want.shape, ambiguous.shape)
    share = float(ambiguous.mean()) if ambiguous.size else 0.0
    assert share <= cap, f'{what}: ambiguous share {share:.4f} ({int(ambiguous.sum())} of {ambiguous.size} rows) exceeds the cap {cap}'
    if np.issubdtype(want.dtype, np.integer):
        bad = np.rint(got.astype(np.float64)).astype(np.int64) != want
        bad |= got != np.rint(got)
    else:
        err = np.abs(got.astype(np.float64) - want)
        bad = ~(err <= VALUE_TOL)
        bad = bad.reshape(bad.shape[0], -1).any(axis=1)
    bad &= ~ambiguous
    rows = np.nonzero(bad)[0]
    assert rows.size == 0, (f'{what}: {rows.size} of {int((~ambiguous).sum())} unambiguous rows differ from the replay; rows '
                            f'{rows[:8].tolist()} got {got[rows[:8]].tolist()} want {want[rows[:8]].tolist()}')
    return share, int((~ambiguous).sum())


# ---- float32 restatements of the kernel arithmetic (the CPU suite's stand-in for the device) ------------------------------------
# `defect`: one of the planted defects of tests/test_draw_reference_host.py, None for the honest restatement.
def honest_f32_categorical(logits, valid, u, mode, defect=None):
    z = np.asarray(logits, dtype=F32)
    valid = np.asarray(valid, dtype=bool)
    if defect == 'masked_counted':
        valid = np.ones_like(valid)
    R, L = z.shape
    u = np.asarray(u, dtype=F32)
    m = np.where(valid, z, F32(-np.inf)).max(axis=1, initial=F32(-np.inf)).astype(F32)
    with np.errstate(invalid='ignore', over='ignore'):  # (masked entries may exceed the maximum of the valid ones)
        e = np.exp((z - m[:, None]).astype(F32)).astype(F32)
    S = np.zeros(R, dtype=F32)
    for i in range(L):
        S = np.where(valid[:, i], S + e[:, i], S).astype(F32)
    if mode == EVAL:
        best, bv = np.zeros(R, dtype=np.int64), np.full(R, F32(-1))
        for i in range(L):
            p = np.where(valid[:, i], e[:, i], F32(0))
            take = p > bv
            best, bv = np.where(take, i, best), np.where(take, p, bv)
        return best
    run = np.zeros(R, dtype=F32)
    last = np.zeros(R, dtype=np.int64)
    pick = np.full(R, -1, dtype=np.int64)
    with np.errstate(invalid='ignore', divide='ignore'):
        for i in range(L):
            v = valid[:, i] & (pick < 0)
            run = np.where(v, run + (e[:, i] / S).astype(F32), run).astype(F32)
            last = np.where(v, i, last)
            pick = np.where(v & (u < run), i, pick)
    pick = np.where(pick < 0, last, pick)
    if defect == 'shifted':
        pick = np.minimum(pick + 1, L - 1)
    return pick


def _f32_gmm_draw(o, logstd, G, half_w, center, u0, u1, u2, defect=None):
    o = np.asarray(o, dtype=F32)
    R = o.shape[0]
    g = honest_f32_categorical(o[:, :G], np.ones((R, G), dtype=bool), u0, TRAIN)
    u1, u2 = np.asarray(u1, dtype=F32), np.asarray(u2, dtype=F32)
    trig = np.sin if defect == 'sin_for_cos' else np.cos
    zn = (np.sqrt(F32(-2) * np.log(u1)) * trig(F32(6.283185307179586) * u2)).astype(F32)
    sd = np.maximum(np.exp(np.asarray(logstd, dtype=F32)), F32(1e-6))[g]
    x = np.tanh(o[np.arange(R), G + g]) * F32(half_w) + F32(center) + sd * zn
    assert x.dtype == F32
    return x


def _f32_gmm_logp(o, logstd, G, half_w, center, x):
    o = np.asarray(o, dtype=F32)
    mx = o[:, :G].max(axis=1)
    se = np.zeros_like(mx)
    for g in range(G):
        se = se + np.exp(o[:, g] - mx)
    lse = mx + np.log(se)
    t = []
    for g in range(G):
        mean = np.tanh(o[:, G + g]) * F32(half_w) + F32(center)
        sd = np.maximum(np.exp(F32(logstd[g])), F32(1e-6))
        d = x - mean
        t.append(-(d * d) / (F32(2) * sd * sd) - np.log(sd) - F32(0.9189385332046727) + (o[:, g] - lse))
    t = np.stack(t, axis=1)
    tm = t.max(axis=1)
    s = np.zeros_like(tm)
    for g in range(G):
        s = s + np.exp(t[:, g] - tm)
    out = tm + np.log(s)
    assert out.dtype == F32
    return out


def honest_f32_gmm(o, logstd, G, half_w, center, u0, u1, u2, defect=None):
    x = _f32_gmm_draw(o, logstd, G, half_w, center, u0, u1, u2, defect)
    return x if defect == 'no_clamp' else np.maximum(x, F32(0.001))


def honest_f32_gmm_best_of(o, logstd, G, half_w, center, seed, samples, count=128, lp_out=None):
    R = np.asarray(o).shape[0]
    best = np.full(R, F32(-np.inf))
    x = np.full(R, F32(center))
    for k in range(count):
        u = [u01(seed, samples, 2, 3 * k + 3 + j) for j in range(3)]
        c = _f32_gmm_draw(o, logstd, G, half_w, center, *u)
        lp = _f32_gmm_logp(o, logstd, G, half_w, center, c)
        if lp_out is not None:
            lp_out.append((c, lp))
        take = lp > best
        best, x = np.where(take, lp, best), np.where(take, c, x)
    return x


def honest_f32_normal3(cout, logstd, half_w, center, u, mode, defect=None):
    cout = np.asarray(cout, dtype=F32)
    mean = np.tanh(cout) * np.asarray(half_w, dtype=F32)[None, :] + np.asarray(center, dtype=F32)[None, :]
    if mode == EVAL:
        return mean
    u = np.asarray(u, dtype=F32)
    trig = np.sin if defect == 'sin_for_cos' else np.cos
    zn = np.sqrt(F32(-2) * np.log(u[:, :, 0])) * trig(F32(6.283185307179586) * u[:, :, 1])
    x = mean + np.exp(F32(1e-6) + np.asarray(logstd, dtype=F32))[None, :] * zn
    if defect != 'no_clamp':
        x[:, 0] = np.maximum(x[:, 0], F32(0.001))
    assert x.dtype == F32
    return x


def ylm25_f32(x, y, z):
    """ylm25 of csrc/common.h on float32 arrays -> (yr, yi) [n][25]"""
    n = x.shape[0]
    yr, yi = np.zeros((n, 25), dtype=F32), np.zeros((n, 25), dtype=F32)
    f = F32
    yr[:, 0] = f(0.28209479177387814)
    c1r, c1i = x, y
    c2r, c2i = x * x - y * y, f(2) * x * y
    c3r, c3i = c2r * x - c2i * y, c2r * y + c2i * x
    c4r, c4i = c2r * c2r - c2i * c2i, f(2) * c2r * c2i
    z2 = z * z

    def pair(qp, qm, q, cr, ci, odd):  # Y_l^m = q c^m, Y_l^-m = (-1)^m conj
        yr[:, qp], yi[:, qp] = q * cr, q * ci
        yr[:, qm], yi[:, qm] = (-q * cr, q * ci) if odd else (q * cr, -q * ci)

    yr[:, 2] = f(0.4886025119029199) * z
    pair(3, 1, f(-0.3454941494713355), c1r, c1i, True)
    yr[:, 6] = f(0.6307831305050401) * f(0.5) * (f(3) * z2 - f(1))
    pair(7, 5, f(0.2575161346821264) * (f(-3) * z), c1r, c1i, True)
    pair(8, 4, f(0.1287580673410632) * f(3), c2r, c2i, False)
    yr[:, 12] = f(0.7463526651802308) * f(0.5) * (f(5) * z2 - f(3)) * z
    pair(13, 11, f(0.21545345607610045) * f(-0.5) * (f(15) * z2 - f(3)), c1r, c1i, True)
    pair(14, 10, f(0.06813236509555216) * f(15) * z, c2r, c2i, False)
    pair(15, 9, f(0.02781492157551894) * f(-15), c3r, c3i, True)
    yr[:, 20] = f(0.8462843753216345) * f(0.125) * ((f(35) * z2 - f(30)) * z2 + f(3))
    pair(21, 19, f(0.18923493915151202) * f(-2.5) * (f(7) * z2 - f(3)) * z, c1r, c1i, True)
    pair(22, 18, f(0.044603102903819275) * f(7.5) * (f(7) * z2 - f(1)), c2r, c2i, False)
    pair(23, 17, f(0.011920680675222404) * f(-105) * z, c3r, c3i, True)
    pair(24, 16, f(0.004214597070904597) * f(105), c4r, c4i, False)
    return yr, yi


def _f32_density(sar, sai, invk, x, y, z):
    yr, yi = ylm25_f32(x, y, z)
    sr, si = np.zeros_like(x), np.zeros_like(x)
    for q in range(25):
        sr = sr + (sar[q] * yr[:, q] - sai[q] * yi[:, q])
        si = si + (sar[q] * yi[:, q] + sai[q] * yr[:, q])
    out = (sr * sr + si * si) * invk
    assert out.dtype == F32
    return out


def honest_f32_so3(coef, has_beta, beta, empty, seed, samples, mode, defect=None, trace=None):
    coef = np.asarray(coef, dtype=F32)
    R, _, CE, _ = coef.shape
    beta = F32(beta if has_beta else 0)
    ngrid = 4096 if has_beta else 1024
    gi = np.arange(ngrid, dtype=F32)
    gct = F32(1) - F32(2) * (gi + F32(0.5)) / F32(ngrid)
    gst = np.sqrt(np.maximum(F32(0), F32(1) - gct * gct))
    gph = F32(6.283185307179586) * gi / F32(1.618033988749895)
    gx, gy = gst * np.cos(gph), gst * np.sin(gph)
    need = 1 if mode == TRAIN else (128 if has_beta else 256)
    if defect == 'best_of_halved' and mode == EVAL:
        need //= 2
    out = np.tile(np.array([0, 0, 1], dtype=F32), (R, 1))
    for r in range(R):
        sar, sai = np.zeros(25, dtype=F32), np.zeros(25, dtype=F32)
        for ce in range(CE):
            sar, sai = sar + coef[r, :, ce, 0], sai + coef[r, :, ce, 1]
        k = F32(0)
        for q in range(25):
            k = k + (sar[q] * sar[q] + sai[q] * sai[q])
        invk = F32(1) / np.maximum(k, F32(1e-10))
        fg = _f32_density(sar, sai, invk, gx, gy, gct)
        vmax = ((-beta * fg) if has_beta else fg).max()
        if defect == 'half_envelope':
            vmax = (vmax - F32(np.log(2))) if has_beta else vmax * F32(0.5)
        accept_all = bool(empty[r]) and not has_beta
        have, best = 0, F32(-np.inf)
        tr_p, tr_v, tr_a = [], [], []
        training_best = defect == 'best_in_training' and mode == TRAIN
        for rnd in range(SO3_MAX_ROUNDS):
            if have >= need:
                break
            i = rnd * 256 + np.arange(256)
            u1, u2, u3 = (u01(seed, samples[r], 3, 3 * i + j) for j in range(3))
            ct = F32(1) - F32(2) * u1
            st = np.sqrt(np.maximum(F32(0), F32(1) - ct * ct))
            ph = F32(6.283185307179586) * u2
            x, y = st * np.cos(ph), st * np.sin(ph)
            f = _f32_density(sar, sai, invk, x, y, ct)
            val = -beta * f if has_beta else f
            if accept_all:
                acc = np.ones(256, dtype=bool)
                p = np.ones(256)
            elif has_beta:
                pe = np.exp(val - vmax)
                assert pe.dtype == F32
                acc, p = u3 < pe, pe.astype(np.float64)
            else:
                acc, p = (u3 * vmax) < f, f.astype(np.float64) / np.float64(vmax)
            scanned = 256
            for c in range(256):
                if not acc[c]:
                    continue
                have += 1
                if (mode == TRAIN and not training_best) or val[c] > best:
                    best = val[c]
                    out[r] = (x[c], y[c], ct[c])
                if have >= need and not (training_best and c < 255):
                    scanned = c + 1
                    break
            tr_p.append(p[:scanned]); tr_v.append(val[:scanned].astype(np.float64)); tr_a.append(acc[:scanned])
        if trace is not None:
            trace.append((np.concatenate(tr_p), np.concatenate(tr_v), np.concatenate(tr_a)))
    return out
