"""The joined weight-gradient launch on the GPU (csrc/gemm_dispatch.inc: flush_dw; csrc/gemm.inc: dw2_tile with n blocks).

The mixed list of tests/test_gemm_dw_join_host.py goes through mg_test_gemm_dw_flush: four groups of <= 32 columns, four wider
ones that join their launch as 32-column n blocks, two that cannot (odd K, X misaligned by 4 bytes) and keep the dword form.  The
shapes are the smallest that can go wrong: N = 100 (last block of 4 columns), N = 65 (a block of one column), N = 49 with 15 rows
(fewer than one MFMA tile of rows), 300 rows (two row chunks of 256), K = 34 / 48 (a partial 32-wide k tile), a concatenated X, dW
and db starting non-zero.  Reference, bound and guard checking are those of tests/gemm_ref.py (float64 product, worst-case
gamma(rows + 4) bound, every float outside [N][K) bit-identical)."""
import ctypes as C

import pytest
import torch

from tests import gemm_ref as gr
from tests.test_gemm_dw_join_host import MIXED, NARROW, WIDE, flush_plan

pytestmark = pytest.mark.gpu

_RUNS = {}


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _upload(ops):
    keep = []
    arr, ws, bs = gr.dw_groups(ops, lambda t: keep.append(t.cuda()) or keep[-1])
    return arr, ws, bs, keep


def _flush(lib, name, groups):
    """(ops, launches, form names, dW after, db after) of one list through mg_test_gemm_dw_flush; run once, shared"""
    from molgym_amd import _lib
    if name not in _RUNS:
        ops = gr.build_dw(gr.Case('dw', list(groups), seed=77))
        arr, ws, bs, keep = _upload(ops)
        mask, n = C.c_uint64(0), C.c_int32(0)
        rc = lib.mg_test_gemm_dw_flush(arr, len(ops), C.byref(mask), C.byref(n), _stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.mg_last_error().decode()
        _RUNS[name] = (ops, n.value, _lib.gemm_form_names(mask.value), [w.cpu() for w in ws], [b.cpu() if b is not None else None for b in bs])
    return _RUNS[name]


@pytest.mark.parametrize('name', ['mixed', 'all_join'])
def test_joined_flush_vs_float64(built_lib, name):
    groups = MIXED if name == 'mixed' else NARROW + WIDE
    ops, launches, forms, ws, bs = _flush(built_lib, name, groups)
    fails = gr.check_dw(ops, ws, bs)
    assert not fails, f'{len(fails)} failures:\n' + '\n'.join(fails[:20])


def test_issued_launches_are_the_planned_ones(built_lib):
    for name, groups, want in (('mixed', MIXED, (2, {'dw2', 'dw'})), ('all_join', NARROW + WIDE, (1, {'dw2', 'dw'}))):
        _, launches, forms, _, _ = _flush(built_lib, name, groups)
        assert (launches, forms) == flush_plan(built_lib, groups, None)   # the process's switches, as the launch had them
        assert (launches, forms) == flush_plan(built_lib, groups) == want  # and the defaults: the suite runs under them


def test_narrow_groups_keep_their_bits(built_lib):
    """a <= 32-column group of <= 256 rows is one workgroup per k tile and one atomic per element onto the previous contents, alone
    or in the joined launch: the same tile, the same sum, the same bits"""
    ops, _, _, ws, bs = _flush(built_lib, 'mixed', MIXED)
    checked = 0
    for i, d in enumerate(MIXED):
        if d.N > 32 or d.rows > 256:
            continue
        arr, w1, b1, keep = _upload(ops[i:i + 1])
        mask = C.c_uint64(0)
        rc = built_lib.mg_test_gemm_dw(arr, 1, C.byref(mask), _stream())
        torch.cuda.synchronize()
        assert rc == 0, built_lib.mg_last_error().decode()
        assert torch.equal(w1[0].cpu().view(torch.int32), ws[i].view(torch.int32)), d
        if d.db:
            assert torch.equal(b1[0].cpu().view(torch.int32), bs[i].view(torch.int32)), d
        checked += 1
    assert checked == 2
