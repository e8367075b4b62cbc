"""mg_fold_rows (include/molgym_hip.h): the ordered fold of per-mini-batch gradient rows against a sequential numpy fold in the
same order -- np.array_equal, no tolerance: both sides do the same IEEE additions in the same order, float32 for the gradient,
float64 for the six statistics.

Rows hold normal x 10^uniform(-3, 3), so the order of the additions shows: the test asserts on the CPU that the fold in reversed k
order differs in at least 10 % of the elements for every total >= 3 (per case where n is large enough for a share to mean
something, n >= 255, and on 4096 elements of the same distribution for every case) -- an order bug cannot pass unnoticed.
Padding rows (k >= total) are NaN and must not reach the sums; guard bands around both outputs must stay intact."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NS = [1, 3, 4, 5, 255, 1027, 185006, 212524]
SHAPES = [(1, 1), (1, 7), (2, 4), (3, 4), (4, 3), (8, 33)]
SENTINEL = -1234.5


def _values(rng, shape, dtype):
    return (rng.standard_normal(shape) * 10.0 ** rng.uniform(-3, 3, shape)).astype(dtype)


def _fold(rows, dtype):
    acc = np.zeros(rows.shape[1], dtype=dtype)
    for k in range(rows.shape[0]):
        acc = acc + rows[k]
    assert acc.dtype == dtype
    return acc


def _reversed_differs(rows):
    return float(np.mean(_fold(rows, np.float32) != _fold(rows[::-1], np.float32)))


@functools.lru_cache(maxsize=None)
def _sensitivity(total):
    return _reversed_differs(_values(np.random.default_rng(900 + total), (total, 4096), np.float32))


def _case(n, world, total, seed):
    """(gathered rows as uint8 [world * per_rank, row bytes], gradient rows [total, n] float32, statistics [total, 6] float64)"""
    from molgym_amd import _lib
    rng = np.random.default_rng(seed)
    per_rank, rb = -(-total // world), _lib.fold_row_bytes(n)
    grads, stats = _values(rng, (total, n), np.float32), _values(rng, (total, 6), np.float64)
    buf = np.empty((world * per_rank, rb), dtype=np.uint8)
    nan_row = np.concatenate([np.full(n, np.nan, dtype=np.float32).view(np.uint8), np.full(6, np.nan).view(np.uint8),
                              np.full(rb - n * 4 - 48, 0xff, dtype=np.uint8)])
    buf[:] = nan_row  # padding rows and the pad bytes of every row
    for k in range(total):
        row = buf[_lib.fold_row_index(k, world, per_rank)]
        row[:n * 4] = grads[k].view(np.uint8)
        row[n * 4:n * 4 + 48] = stats[k].view(np.uint8)
    return buf, grads, stats


def _run(built_lib, n, world, total, buf, front=4):
    """grad_out sits `front` floats into a sentinel-filled buffer (4: 16-byte aligned), stats_out two doubles into another"""
    from molgym_amd import _lib
    rows = torch.from_numpy(buf).cuda()
    gbuf = torch.full((front + n + 4, ), SENTINEL, dtype=torch.float32, device='cuda')
    sbuf = torch.full((2 + 6 + 2, ), SENTINEL, dtype=torch.float64, device='cuda')
    _lib.check(built_lib.mg_fold_rows(n, world, -(-total // world), total, C.c_void_p(rows.data_ptr()), buf.shape[1],
                                      C.c_void_p(gbuf.data_ptr() + 4 * front), C.c_void_p(sbuf.data_ptr() + 16),
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    g, s = gbuf.cpu().numpy(), sbuf.cpu().numpy()
    assert np.all(g[:front] == SENTINEL) and np.all(g[front + n:] == SENTINEL)
    assert np.all(s[:2] == SENTINEL) and np.all(s[8:] == SENTINEL)
    return g[front:front + n], s[2:8]


@pytest.mark.parametrize('world,total', SHAPES)
@pytest.mark.parametrize('n', NS)
def test_fold_equals_the_sequential_fold_bit_for_bit(built_lib, n, world, total):
    buf, grads, stats = _case(n, world, total, seed=n * 100 + world * 10 + total)
    if total >= 3:  # the inputs are sensitive to the order
        assert _sensitivity(total) >= 0.10, _sensitivity(total)
        if n >= 255:
            assert _reversed_differs(grads) >= 0.10, _reversed_differs(grads)
    got_g, got_s = _run(built_lib, n, world, total, buf)
    assert np.isfinite(got_g).all() and np.isfinite(got_s).all()  # no NaN of a padding row
    assert np.array_equal(got_g, _fold(grads, np.float32))
    assert np.array_equal(got_s, _fold(stats, np.float64))


@pytest.mark.parametrize('n', [5, 1027])
def test_output_at_a_4_byte_boundary(built_lib, n):
    """grad_out need not be 16-byte aligned (rows must be)"""
    buf, grads, stats = _case(n, 3, 7, seed=n)
    for front in (1, 2, 3):
        got_g, got_s = _run(built_lib, n, 3, 7, buf, front=front)
        assert np.array_equal(got_g, _fold(grads, np.float32)) and np.array_equal(got_s, _fold(stats, np.float64))


def test_outputs_are_overwritten_and_an_empty_fold_is_zero(built_lib):
    buf, _, _ = _case(9, 2, 3, seed=1)
    got_g, got_s = _run(built_lib, 9, 2, 0, buf)  # (total = 0 of 2 x 2 gathered rows: nothing is read)
    assert np.array_equal(got_g, np.zeros(9, dtype=np.float32)) and np.array_equal(got_s, np.zeros(6))
    assert not np.signbit(got_g).any()  # +0.0


def test_bad_arguments_are_refused(built_lib):
    from molgym_amd import _lib
    rows = torch.zeros(4, _lib.fold_row_bytes(8), dtype=torch.uint8, device='cuda')
    g, s = torch.zeros(8, device='cuda'), torch.zeros(6, dtype=torch.float64, device='cuda')
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rb = rows.shape[1]
    assert built_lib.mg_fold_rows(8, 2, 2, 5, P(rows), rb, P(g), P(s), st) != 0       # more rows than were gathered
    assert built_lib.mg_fold_rows(8, 2, 2, 4, P(rows), rb - 8, P(g), P(s), st) != 0   # stride not a multiple of 16
    assert built_lib.mg_fold_rows(8, 2, 2, 4, P(rows), 64, P(g), P(s), st) != 0       # stride below a row
    assert built_lib.mg_fold_rows(8, 2, 1, 2, P(rows, 4), rb, P(g), P(s), st) != 0    # rows not 16-byte aligned
    assert built_lib.mg_fold_rows(8, 0, 2, 0, P(rows), rb, P(g), P(s), st) != 0       # world < 1
    _lib.check(built_lib.mg_fold_rows(8, 2, 2, 4, P(rows), rb, P(g), P(s), st))
    torch.cuda.synchronize()
