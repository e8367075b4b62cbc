"""The one-round body of the 16-way row form (csrc/gemm.inc: k_gemm_mfma_rows_or, behind MG_FORM_ROWS_W16) through mg_test_gemm_mt.

One workgroup per LIVE 16-row tile on a flat grid, eight waves over the reduction blocks, the weight operands either as 16-byte
loads from the transposed copy Mt [N][ldmt] or as dword loads from M.  Every call here is one launch of several groups of unequal
row counts (an empty one among them), so the flat grid and the empty-group filter are part of every case.  Checked per call:
  * outputs within the derived bound of the float64 reference (tests/gemm_ref.py, imported as is), guard rows and pad columns of Y
    bit-identical;
  * with Mt == without Mt, bit for bit, and the same call twice, bit for bit;
  * forms_out == {rows_w16}, also with MG_ROWS_W16_ONEROUND=0 (the 16-wave body under the same bit), which meets the same bound --
    and gives the same bits: the one-round body keeps the sixteen partial sums of the 16-wave body and their order;
  * X and Mt come back untouched.  Behind the last row of every Mt sits a guard row of NaNs, and its pad columns [R, ldmt) are NaNs
    too: a weight read past R or past row N - 1 cannot hide behind a zero X.  The floats behind every X are 1e4 (gemm_ref._matrix)."""
import ctypes as C

import pytest
import torch

from tests import gemm_ref as gr

pytestmark = pytest.mark.gpu

ROWS = (17, 0, 140, 1, 16, 15)          # five live groups of unequal row counts and an empty one, in this order in every call
R_ALL = (160, 164, 172, 220, 704)       # 10 blocks: fewer than partial sums; partial last block; three quads in it; one trip per wave; three
N_ALL = (1, 16, 17, 20, 32, 33, 48)     # one to three column tiles, the clamp at N - 1, four live columns in the second tile
# per group of a call: pitches of X and Mt beyond R, epilogue flags
VARIANTS = (dict(ldx_pad=(12, ), bias=True), dict(), dict(ldx_pad=(4, ), rowscale=True), dict(acc=True), dict(ldx_pad=(8, ), bias=True, acc=True),
            dict(rowscale=True))
MT_PAD = (4, 0, 0, 8, 0, 4)


def _case(R, N, seed):
    return gr.Case('gemm', [gr.G(rows, N, R, **VARIANTS[i]) for i, rows in enumerate(ROWS)], seed=seed)


def _mixed_case():
    """groups of different R, N and segment counts in one call: three column-tile widths on one grid, a short reduction beside the
    long ones, two segments (never with Mt)"""
    return gr.Case('gemm', [gr.G(140, 20, 220, bias=True), gr.G(15, 3, 8), gr.G(65, 32, 704, acc=True), gr.G(1, 17, 164),
                            gr.G(33, 48, 172, nseg=2, ldx_pad=(0, 4), rowscale=True), gr.G(0, 20, 160), gr.G(100, 33, 160, ldx_pad=(4, ))],
                   seed=977)


def _transposed(o, pad):
    """flat [N + 1][ldmt] buffer: rows 0..N-1 = M[0]^T in the first R columns, everything else (pad columns, the guard row) NaN"""
    g = o['g']
    ldmt = g.R + pad
    flat = gr._sentinel((g.N + 1) * ldmt)
    flat[:g.N * ldmt].view(g.N, ldmt)[:, :g.R] = o['M'][0][1][:, :g.N].t()
    return flat, ldmt


def _call(lib, ops, with_mt, switches=None):
    """one mg_test_gemm_mt call on fresh uploads; returns (forms_out, Y buffers on the CPU, failures of the untouched-input check)"""
    keep = []
    arr, ys = gr.gemm_groups(ops, lambda t: keep.append((t, t.cuda())) or keep[-1][1])
    n = len(ops)
    mts, ldmt = (C.c_void_p * n)(), (C.c_int32 * n)()
    for i, o in enumerate(ops):
        if with_mt and o['g'].nseg == 1 and o['g'].rows > 0:
            flat, ld = _transposed(o, MT_PAD[i % len(MT_PAD)])
            keep.append((flat, flat.cuda()))
            mts[i], ldmt[i] = keep[-1][1].data_ptr(), ld
    mask = C.c_uint64(0)
    rc = lib.mg_test_gemm_mt(arr, mts, ldmt, n, switches, C.byref(mask), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0, lib.mg_last_error().decode()
    placed_y = {id(y) for y in ys}
    touched = [f'input {j} was written' for j, (cpu, dev) in enumerate(keep)
               if id(dev) not in placed_y and not torch.equal(cpu.view(torch.int32), dev.cpu().view(torch.int32))]
    return mask.value, [y.cpu() for y in ys], touched


def _check(lib, case):
    from molgym_amd import _lib
    ops = gr.build_gemm(case)
    form = {'rows_w16'}
    m_mt, y_mt, bad_mt = _call(lib, ops, True)
    m_m, y_m, bad_m = _call(lib, ops, False)
    m_again, y_again, _ = _call(lib, ops, True)
    m_old, y_old, bad_old = _call(lib, ops, True, b'MG_ROWS_W16_ONEROUND=0')
    fails = bad_mt + bad_m + bad_old
    for what, m in (('Mt', m_mt), ('M', m_m), ('repeat', m_again), ('MG_ROWS_W16_ONEROUND=0', m_old)):
        if _lib.gemm_form_names(m) != form:
            fails.append(f'{what}: launched {sorted(_lib.gemm_form_names(m))}')
    fails += [f'Mt: {f}' for f in gr.check_gemm(ops, y_mt)]
    fails += [f'MG_ROWS_W16_ONEROUND=0: {f}' for f in gr.check_gemm(ops, y_old)]
    for i, (a, d) in enumerate(zip(y_mt, y_old)):
        if not torch.equal(a.view(torch.int32), d.view(torch.int32)):
            fails.append(f'group {i}: MG_ROWS_W16_ONEROUND=0 and 1 differ in {int((a.view(torch.int32) != d.view(torch.int32)).sum())} floats')
    for i, (a, b, c) in enumerate(zip(y_mt, y_m, y_again)):
        if not torch.equal(a.view(torch.int32), b.view(torch.int32)):
            fails.append(f'group {i}: the outputs with and without Mt differ in {int((a.view(torch.int32) != b.view(torch.int32)).sum())} floats')
        if not torch.equal(a.view(torch.int32), c.view(torch.int32)):
            fails.append(f'group {i}: the same call twice differs in {int((a.view(torch.int32) != c.view(torch.int32)).sum())} floats')
    return fails


@pytest.mark.parametrize('R', R_ALL)
@pytest.mark.parametrize('N', N_ALL)
def test_rows_oneround_vs_float64(built_lib, R, N):
    fails = _check(built_lib, _case(R, N, seed=7000 + 64 * R + N))
    assert not fails, f'{len(fails)} failures:\n' + '\n'.join(fails[:20])


def test_rows_oneround_mixed_groups(built_lib):
    fails = _check(built_lib, _mixed_case())
    assert not fails, f'{len(fails)} failures:\n' + '\n'.join(fails[:20])
