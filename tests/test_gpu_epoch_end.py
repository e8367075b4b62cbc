"""The kernels that end a PPO epoch, each called directly on vectors of fixed seed and held to numpy in float64 (or to float32
arithmetic restated in numpy where the kernel's own rounding is the contract):

  B1  mg_ppo_epoch_end: the record, the clip, the KL test (>, not >=; NaN does not stop), the latching stop flag and the clip that a
      stopped epoch must skip -- at n = 1, block_sum's 255 | 256 | 257, k_sumsq's one-block | several-block seam 2048 | 2049 and its
      capped grid (530000 > 256 workgroups x 2048 elements: the grid-stride loop)
  B2  mg_adam_step_gated against mg_adam_step, and the two chained on one stream as ppo.train issues them
  B3  mg_grad_norm_clip at the same sizes, and k_sumsq_ord (deterministic mode) around its stride of 1024
  B4  mg_gae around its 64-path workgroups, with paths of length 0
  B5  mg_adv_normalize around its 256-thread stride, and at a mean of 1e6 where only the two-pass form keeps its digits

Bounds: the norm's 1e-5 is what tests/test_gpu_ppo.py::test_grad_norm_and_clip holds this float32 sum to; GAE and the normalisation
keep that file's float64 bounds; everything else is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

from molgym_amd import _lib
from oracle.ppo_ref import gae_ref, normalize_adv_ref
from tests.helpers import launch_log

pytestmark = pytest.mark.gpu
P = lambda t: C.c_void_p(t.data_ptr())
S = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
SIZES = [1, 255, 256, 257, 2048, 2049, 530000]
F32 = np.float32


def _vector(n, seed):
    return (0.3 * np.random.default_rng(seed).standard_normal(n)).astype(F32)


def _norm64(g):
    return float(np.linalg.norm(g.astype(np.float64)))


def _clipped(g, max_norm, norm):
    """clip_grad_norm_'s scaling in float32, from the norm the kernel itself reported (k_clip_scale / k_epoch_end)"""
    coef = F32(max_norm) / (F32(norm) + F32(1e-6))
    assert coef < 1.0
    return g * coef


def _same_bits(t, want):
    got = t.cpu().numpy()
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def _epoch_end(lib, g, max_norm, accum, inv_m, kl_limit, flag):
    """one mg_ppo_epoch_end -> (rec as numpy, the gradient tensor, the flag tensor); `flag`: the value the flag holds before"""
    grad = torch.from_numpy(g.copy()).cuda()
    acc = torch.from_numpy(np.asarray(accum, dtype=np.float64)).cuda()
    rec = torch.full((8, ), -7.0, dtype=torch.float64, device='cuda')
    stop = torch.full((1, ), int(flag), dtype=torch.int32, device='cuda')
    scratch = torch.full((1, ), float('nan'), dtype=torch.float32, device='cuda')
    _lib.check(lib.mg_ppo_epoch_end(g.size, P(grad), max_norm, P(acc), inv_m, kl_limit, P(rec), P(stop), P(scratch), S()), lib)
    torch.cuda.synchronize()
    assert _same_bits(acc, np.asarray(accum, dtype=np.float64))   # (read only)
    return rec.cpu().numpy(), grad, stop


ACCUM = np.array([-0.31, -0.042, 0.77, 0.418, 0.0123, 1.7])   # three mini-batches' share x statistics, summed


# ---- B1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', SIZES)
def test_epoch_end_record_and_clip(built_lib, n):
    g = _vector(n, seed=n)
    want = _norm64(g)
    inv_m = 1.0 / 3.0
    # not stopped, max_norm below the norm: clipped by the float32 coefficient, the PRE-clip norm reported
    rec, grad, stop = _epoch_end(built_lib, g, 0.5 * want, ACCUM, inv_m, 1e9, 0)
    assert (rec[:6] == ACCUM * inv_m).all(), rec
    assert abs(rec[6] - want) <= 1e-5 * want and rec[7] == 0.0 and stop.item() == 0
    assert float(F32(rec[6])) == rec[6]
    assert _same_bits(grad, _clipped(g, 0.5 * want, rec[6]))
    # max_norm above the norm, and no clip asked for: the bytes stay, the norm is reported all the same
    for max_norm in (2.0 * want, 0.0):
        rec, grad, stop = _epoch_end(built_lib, g, max_norm, ACCUM, 1.0, 1e9, 0)
        assert (rec[:6] == ACCUM).all() and abs(rec[6] - want) <= 1e-5 * want and rec[7] == 0.0 and stop.item() == 0
        assert _same_bits(grad, g)


@pytest.mark.parametrize('n', [257, 2049])
def test_epoch_end_kl_test_and_latch(built_lib, n):
    g = _vector(n, seed=10 + n)
    want = _norm64(g)
    max_norm = 0.5 * want            # (norm > max_norm throughout: an epoch that is not stopped IS clipped)
    inv_m = 1.0 / 3.0                # three accumulated mini-batches
    kl = float(ACCUM[4] * inv_m)
    below, above = float(np.nextafter(kl, -np.inf)), float(np.nextafter(kl, np.inf))
    # KL just above the limit: stop, the flag set, the gradient untouched although norm > max_norm
    rec, grad, stop = _epoch_end(built_lib, g, max_norm, ACCUM, inv_m, below, 0)
    assert rec[7] == 1.0 and stop.item() == 1 and _same_bits(grad, g)
    assert (rec[:6] == ACCUM * inv_m).all() and abs(rec[6] - want) <= 1e-5 * want
    # exactly the limit, and just below it: the reference's test is `>`
    for limit in (kl, above):
        rec, grad, stop = _epoch_end(built_lib, g, max_norm, ACCUM, inv_m, limit, 0)
        assert rec[7] == 0.0 and stop.item() == 0 and _same_bits(grad, _clipped(g, max_norm, rec[6])), limit
    # the same sum with one mini-batch's share: the limit is compared with accum x inv_m, not with accum
    rec, grad, stop = _epoch_end(built_lib, g, max_norm, ACCUM, 1.0, kl, 0)
    assert rec[7] == 1.0 and stop.item() == 1 and rec[4] == ACCUM[4] and _same_bits(grad, g)
    # NaN compares false, as `approx_kl > 1.5 * target_kl` does: no stop
    nan = ACCUM.copy()
    nan[4] = np.nan
    rec, grad, stop = _epoch_end(built_lib, g, max_norm, nan, inv_m, 0.0, 0)
    assert rec[7] == 0.0 and stop.item() == 0 and np.isnan(rec[4]) and (rec[[0, 1, 2, 3, 5]] == (nan * inv_m)[[0, 1, 2, 3, 5]]).all()
    assert _same_bits(grad, _clipped(g, max_norm, rec[6]))
    # the latch: once set, an epoch of KL 0 under any limit stays stopped and unclipped
    calm = ACCUM.copy()
    calm[4] = 0.0
    for flag in (1, 5):
        rec, grad, stop = _epoch_end(built_lib, g, max_norm, calm, inv_m, 1e9, flag)
        assert rec[7] == 1.0 and stop.item() == 1 and _same_bits(grad, g) and abs(rec[6] - want) <= 1e-5 * want
    # two calls on ONE flag, as an epoch follows another: the first stops, the second finds the flag
    grad = torch.from_numpy(g.copy()).cuda()
    rec = torch.zeros(8, dtype=torch.float64, device='cuda')
    stop = torch.zeros(1, dtype=torch.int32, device='cuda')
    scratch = torch.zeros(1, device='cuda')
    for accum, limit in ((ACCUM, below), (calm, 1e9)):
        acc = torch.from_numpy(accum).cuda()
        _lib.check(built_lib.mg_ppo_epoch_end(n, P(grad), max_norm, P(acc), inv_m, limit, P(rec), P(stop), P(scratch), S()))
        torch.cuda.synchronize()
        assert rec[7].item() == 1.0 and stop.item() == 1 and _same_bits(grad, g)
    assert rec[4].item() == 0.0


def test_epoch_end_null_arguments(built_lib):
    grad, acc = torch.zeros(4, device='cuda'), torch.zeros(6, dtype=torch.float64, device='cuda')
    rec, stop = torch.zeros(8, dtype=torch.float64, device='cuda'), torch.zeros(1, dtype=torch.int32, device='cuda')
    scratch = torch.zeros(1, device='cuda')
    args = [P(grad), P(acc), P(rec), P(stop), P(scratch)]
    for k in range(5):
        a = list(args)
        a[k] = None
        rc = built_lib.mg_ppo_epoch_end(4, a[0], 0.5, a[1], 1.0, 1e9, a[2], a[3], a[4], S())
        assert rc == -1 and 'null argument' in built_lib.mg_last_error().decode(), (k, rc)
    torch.cuda.synchronize()
    assert not grad.any() and not rec.any() and not stop.any()


# ---- B2 ---------------------------------------------------------------------------------------------------------------------
HP = dict(lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0)


def _adam_state(n, amsgrad, seed):
    rng = np.random.default_rng(seed)
    t = lambda x: torch.from_numpy(x.astype(F32)).cuda()
    st = [t(rng.standard_normal(n)), t(0.1 * rng.standard_normal(n)), t(0.01 * rng.standard_normal(n)),
          t(1e-4 * rng.random(n))]
    st.append(t(1e-4 * rng.random(n)) if amsgrad else None)
    return st   # param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq


def _adam(lib, st, step, flag=None, gated=True):
    p, g, m, v, vmax = st
    n = p.numel()
    head = (n, P(p), P(g), P(m), P(v), None if vmax is None else P(vmax), HP['lr'], HP['beta1'], HP['beta2'], HP['eps'], HP['wd'], step, 0)
    if gated:
        _lib.check(lib.mg_adam_step_gated(*head, None if flag is None else P(flag), S()), lib)
    else:
        _lib.check(lib.mg_adam_step(*head, S()), lib)
    torch.cuda.synchronize()


def _clone(st):
    return [None if t is None else t.clone() for t in st]


def _equal(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('n', [1, 255, 257, 4099])
@pytest.mark.parametrize('amsgrad', [False, True])
@pytest.mark.parametrize('step', [1, 7])
def test_gated_adam_step(built_lib, n, amsgrad, step):
    start = _adam_state(n, amsgrad, seed=n + step)
    plain = _clone(start)
    _adam(built_lib, plain, step, gated=False)
    assert not torch.equal(plain[0], start[0]) and not torch.equal(plain[2], start[2]) and torch.equal(plain[1], start[1])
    for flag_value in (0, None):      # a zero flag and no flag at all: mg_adam_step
        got = _clone(start)
        _adam(built_lib, got, step, None if flag_value is None else torch.zeros(1, dtype=torch.int32, device='cuda'))
        assert _equal(got, plain), flag_value
    for flag_value in (1, -3):        # any non-zero flag: nothing moves
        got = _clone(start)
        flag = torch.full((1, ), flag_value, dtype=torch.int32, device='cuda')
        _adam(built_lib, got, step, flag)
        assert _equal(got, start) and flag.item() == flag_value, flag_value


@pytest.mark.parametrize('n', [257, 4099])
@pytest.mark.parametrize('stops', [True, False])
def test_epoch_end_then_gated_adam_on_one_stream(built_lib, n, stops):
    """mg_ppo_epoch_end and mg_adam_step_gated issued back to back, nothing waited for in between (ppo.train): an epoch over the
    KL limit leaves theta and the moments untouched; another leaves them equal to clip, then mg_adam_step"""
    start = _adam_state(n, True, seed=3 * n)
    g = start[1].cpu().numpy()
    max_norm = 0.5 * _norm64(g)
    kl = float(ACCUM[4] / 3.0)
    got = _clone(start)
    acc = torch.from_numpy(ACCUM).cuda()
    rec = torch.zeros(8, dtype=torch.float64, device='cuda')
    stop = torch.zeros(1, dtype=torch.int32, device='cuda')
    scratch = torch.zeros(1, device='cuda')
    p, grad, m, v, vmax = got
    _lib.check(built_lib.mg_ppo_epoch_end(n, P(grad), max_norm, P(acc), 1.0 / 3.0, kl * (0.5 if stops else 2.0), P(rec), P(stop), P(scratch), S()))
    _lib.check(built_lib.mg_adam_step_gated(n, P(p), P(grad), P(m), P(v), P(vmax), HP['lr'], HP['beta1'], HP['beta2'], HP['eps'], HP['wd'],
                                            3, 0, P(stop), S()))
    torch.cuda.synchronize()
    assert rec[7].item() == (1.0 if stops else 0.0) and stop.item() == (1 if stops else 0)
    if stops:
        assert _equal(got, start)
        return
    want = _clone(start)
    want[1] = torch.from_numpy(_clipped(g, max_norm, rec[6].item())).cuda()
    assert torch.equal(grad, want[1])
    _adam(built_lib, want, 3, gated=False)
    assert _equal(got, want) and not torch.equal(got[0], start[0])


def test_agent_adam_step_with_skip_flag_and_unstep(built_lib):
    """FlatThetaAgent.adam_step(opt, skip_flag=...) advances the optimizer's counters whether or not the device skips the update;
    adam_unstep takes a skipped step back"""
    from tests.helpers import make_pair
    ac, _, _ = make_pair('cfg2', seed=5)
    opt = torch.optim.Adam(ac.parameters(), lr=3e-4, amsgrad=True)
    ac.theta.grad = torch.randn(ac.theta.numel(), generator=torch.Generator().manual_seed(1)).cuda()
    flag = torch.zeros(1, dtype=torch.int32, device='cuda')
    assert ac.adam_step(opt, skip_flag=flag) is True
    torch.cuda.synchronize()
    st = opt.state[ac.theta]
    assert float(st['step']) == 1.0
    keep = {k: st[k].clone() for k in ('exp_avg', 'exp_avg_sq', 'max_exp_avg_sq')}
    theta, count = ac.theta.detach().clone(), getattr(opt, '_step_count', None)
    flag.fill_(1)
    assert ac.adam_step(opt, skip_flag=flag) is True
    torch.cuda.synchronize()
    assert float(st['step']) == 2.0 and torch.equal(ac.theta.detach(), theta) and all(torch.equal(st[k], keep[k]) for k in keep)
    ac.adam_unstep(opt, 1)
    assert float(st['step']) == 1.0 and getattr(opt, '_step_count', None) == count
    flag.zero_()
    assert ac.adam_step(opt, skip_flag=flag) is True   # the next real step is number 2
    torch.cuda.synchronize()
    assert float(st['step']) == 2.0 and not torch.equal(ac.theta.detach(), theta)


# ---- B3 ---------------------------------------------------------------------------------------------------------------------
def _norm_clip(lib, g, max_norm):
    grad = torch.from_numpy(g.copy()).cuda()
    out = torch.full((2, ), float('nan'), dtype=torch.float32, device='cuda')
    _lib.check(lib.mg_grad_norm_clip(g.size, P(grad), max_norm, P(out), S()), lib)
    torch.cuda.synchronize()
    return out[0].item(), grad


def _check_norm_clip(lib, g):
    want = _norm64(g)
    norm, grad = _norm_clip(lib, g, 0.5 * want)
    assert abs(norm - want) <= 1e-5 * want and _same_bits(grad, _clipped(g, 0.5 * want, norm))
    for max_norm in (2.0 * want, 0.0):
        norm, grad = _norm_clip(lib, g, max_norm)
        assert abs(norm - want) <= 1e-5 * want and _same_bits(grad, g)
    return norm


@pytest.mark.parametrize('n', SIZES)
def test_grad_norm_clip_sizes(built_lib, n):
    with launch_log(built_lib) as log:
        _check_norm_clip(built_lib, _vector(n, seed=20 + n))
    assert log.ran('k_sumsq') and not log.ran('k_sumsq_ord')


@pytest.mark.parametrize('n', [1, 1023, 1024, 1025, 4097])
def test_grad_norm_clip_ordered_sum(built_lib, n):
    """deterministic mode: k_sumsq_ord, one workgroup of 1024 with a fixed stride -- the same bits every run"""
    g = _vector(n, seed=30 + n)
    prev = built_lib.mg_set_deterministic(1)
    try:
        with launch_log(built_lib) as log:
            first = _check_norm_clip(built_lib, g)
        assert log.ran('k_sumsq_ord') and not log.ran('k_sumsq')
        again, _ = _norm_clip(built_lib, g, 0.0)
        assert F32(first).tobytes() == F32(again).tobytes()
        rec, grad, stop = _epoch_end(built_lib, g, 0.0, ACCUM, 1.0, 1e9, 0)   # the epoch's end takes the same sum
        assert F32(rec[6]).tobytes() == F32(first).tobytes() and _same_bits(grad, g)
    finally:
        built_lib.mg_set_deterministic(prev)


# ---- B4 ---------------------------------------------------------------------------------------------------------------------
GUARD = -12345.0625


def _gae_case(lib, lengths, seed, gamma=0.99, lam=0.97):
    rng = np.random.default_rng(seed)
    lengths = np.asarray(lengths, dtype=np.int64)
    n_paths, T = len(lengths), int(lengths.sum())
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    rew, val, last = rng.standard_normal(T), rng.standard_normal(T), rng.standard_normal(n_paths)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_off, d_rew, d_val, d_last = dev(off), dev(np.append(rew, 0.0)), dev(np.append(val, 0.0)), dev(last)   # (T may be 0)
    adv = torch.full((T + 16, ), GUARD, dtype=torch.float64, device='cuda')
    ret = torch.full((T + 16, ), GUARD, dtype=torch.float64, device='cuda')
    _lib.check(lib.mg_gae(n_paths, P(d_off), P(d_rew), P(d_val), P(d_last), gamma, lam, P(adv[8:]), P(ret[8:]), S()), lib)
    torch.cuda.synchronize()
    want_a, want_r = np.full(T + 16, GUARD), np.full(T + 16, GUARD)
    for p in range(n_paths):
        t0, t1 = off[p], off[p + 1]
        if t1 > t0:
            want_a[8 + t0:8 + t1], want_r[8 + t0:8 + t1] = gae_ref(rew[t0:t1], val[t0:t1], last[p], gamma, lam)
    got_a, got_r = adv.cpu().numpy(), ret.cpu().numpy()
    for got, want in ((got_a, want_a), (got_r, want_r)):
        assert (got[:8] == GUARD).all() and (got[-8:] == GUARD).all()                     # the padding on either side
        np.testing.assert_allclose(got[8:8 + T], want[8:8 + T], rtol=1e-12, atol=1e-14)  # (no slot kept its guard value either)
    return T


@pytest.mark.parametrize('n_paths', [1, 63, 64, 65, 200])
def test_gae_path_counts_and_empty_paths(built_lib, n_paths):
    """one thread per path, 64 to a workgroup.  A path of length 0 writes nothing: its neighbours' slots hold their own values
    and, where every path is empty, nothing but guard values is left"""
    if n_paths == 1:
        assert _gae_case(built_lib, [37], seed=1) == 37
        assert _gae_case(built_lib, [0], seed=2) == 0
        return
    rng = np.random.default_rng(40 + n_paths)
    lengths = rng.choice([0, 1, 2, 37], size=n_paths)
    lengths[[0, n_paths // 2, n_paths - 1]] = 0          # empty paths at both ends and in the middle ...
    lengths[[1, n_paths - 2]] = [37, 1]                   # ... next to paths that are not
    assert set(lengths.tolist()) == {0, 1, 2, 37}
    _gae_case(built_lib, lengths, seed=n_paths)
    _gae_case(built_lib, np.zeros(n_paths, dtype=np.int64), seed=n_paths + 1)


# ---- B5 ---------------------------------------------------------------------------------------------------------------------
def _normalize(lib, adv):
    d = torch.from_numpy(np.concatenate([[GUARD], adv, [GUARD]])).cuda()
    _lib.check(lib.mg_adv_normalize(adv.size, P(d[1:]), None, S()), lib)
    torch.cuda.synchronize()
    got = d.cpu().numpy()
    assert got[0] == GUARD and got[-1] == GUARD
    return got[1:-1]


@pytest.mark.parametrize('T', [2, 255, 256, 257, 1000])
def test_adv_normalize_sizes(built_lib, T):
    adv = 0.7 + 3.0 * np.random.default_rng(50 + T).standard_normal(T)
    np.testing.assert_allclose(_normalize(built_lib, adv), normalize_adv_ref(adv), rtol=1e-11, atol=1e-13)


def test_adv_normalize_keeps_its_digits_at_a_large_mean(built_lib):
    """mean 1e6, spread 1.  In general the mean of T such numbers carries an error of 1e6 x 2^-53 x T against a spread of 1, in
    the kernel and in numpy alike; here the values are multiples of 2^-10 and T = 1024, so every sum -- and the mean -- is exact
    in float64 in any order, the deviations are exact, and both sides are good to a few ulp: rtol 1e-9 with no absolute term.  A
    one-pass sum of squares (1e12 per term, rounded to 2^-13) would be off by 1e-6."""
    T = 1024
    k = np.rint(1024.0 * np.random.default_rng(7).standard_normal(T))
    adv = 1.0e6 + k / 1024.0
    assert (adv - 1.0e6 == k / 1024.0).all() and abs(adv.std() - 1.0) < 0.1
    np.testing.assert_allclose(_normalize(built_lib, adv), normalize_adv_ref(adv), rtol=1e-9, atol=0.0)
