"""The ordered weight-gradient GEMM form of deterministic mode (csrc/gemm.inc: k_gemm_dw_ord_partial / k_gemm_dw_ord_fold),
called directly through mg_test_gemm_dw_ordered.

Operands, float64 reference, bound and guard checking are those of tests/gemm_ref.py (the bound of reference_dw holds for ANY
order of the additions, so it holds for chunk partials folded in index order).  Beyond parity the form promises bits: the same
call gives the same result every time, a group's result does not depend on what else the call holds or on how the call is cut
into launches, and groups that share a destination give what successive calls give.

C = 64 is the form's minimum row chunk (DWO_MIN_ROWS); chunks start to grow above 64 * 64 = 4096 rows (DWO_MAX_CHUNKS)."""
import ctypes as C

import pytest
import torch

from tests import gemm_ref as gr

pytestmark = pytest.mark.gpu

CHUNK = 64
NS = (1, 3, 33, 128, 129)
KS = (2, 31, 57, 64, 128)
ROWS = (1, 15, 64, 140, 420, CHUNK - 1, CHUNK + 1, 2 * CHUNK + 17, 64 * CHUNK + 3)  # (C itself is the 64 of the first five)
MG_EINVAL = -1


def _ptr(t, off=0):
    return C.c_void_p(t.data_ptr() + 4 * off)


def _upload(ops, share=None):
    """device copies of the operands of build_dw and the descriptor array; share = {group index: group index whose dW / db it uses}"""
    from molgym_amd import _lib
    keep, arr = [], (_lib.GemmDwGroup * len(ops))()
    ws, bs = [], []
    for i, (a, o) in enumerate(zip(arr, ops)):
        d = o['g']
        dev = lambda t: keep.append(t.cuda()) or keep[-1]
        a.dY = _ptr(dev(o['dY'][0]))
        a.X = _ptr(dev(o['X'][0][0]), d.x_off)
        a.ldx = o['X'][0][2]
        if d.cat is not None:
            a.X1, a.ldx1, a.ks1 = _ptr(dev(o['X'][1][0])), o['X'][1][2], d.cat[0]
            a.X2, a.ldx2, a.ks2 = _ptr(dev(o['X'][2][0])), o['X'][2][2], d.cat[1]
        if share and i in share:
            ws.append(ws[share[i]])
            bs.append(bs[share[i]])
        else:
            ws.append(dev(o['dW']))
            bs.append(dev(o['db']) if d.db else None)
        a.dW = _ptr(ws[-1], o['w_base'])
        a.db = _ptr(bs[-1], o['b_base']) if d.db else None
        a.ldy, a.ldw, a.N, a.K, a.rows = o['ldy'], o['ldw'], d.N, d.K, d.rows
    return arr, ws, bs, keep


def _call(lib, arr, n, first=0, scratch_bytes=None):
    """mg_test_gemm_dw_ordered over arr[first : first + n] with the scratch the library asks for (or `scratch_bytes`)"""
    from molgym_amd import _lib
    sub = (_lib.GemmDwGroup * n).from_buffer(arr, first * C.sizeof(_lib.GemmDwGroup))
    if scratch_bytes is None:
        nbytes = C.c_size_t(0)
        rc = lib.mg_gemm_dw_ordered_scratch_bytes(sub, n, C.byref(nbytes))
        if rc != 0:
            return rc
        scratch_bytes = nbytes.value
    # (NaN-filled: a partial tile that pass 1 failed to store would poison the fold)
    scratch = torch.full((scratch_bytes // 4 + 4, ), float('nan'), dtype=torch.float32, device='cuda')
    rc = lib.mg_test_gemm_dw_ordered(sub, n, _ptr(scratch), scratch_bytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def _bits(t):
    return t.view(torch.int32).clone()


@pytest.fixture(autouse=True)
def _switch_off(built_lib):
    """the entry point runs the ordered form whatever the switch says; these tests leave it off"""
    from molgym_amd import _lib
    prev = _lib.set_deterministic(False)
    yield
    _lib.set_deterministic(prev)


@pytest.mark.parametrize('db', [False, True])
@pytest.mark.parametrize('rows', ROWS)
def test_parity_with_float64(built_lib, rows, db):
    """every N x K of the grid as the 25 groups of ONE call (so the call is also cut into launches of 32 groups by the dispatcher's
    own rule when db adds scratch): within reference_dw's bound, nothing outside [N][0..K) written; odd pitches, a misaligned X and
    a non-zero previous dW for every second group"""
    groups = []
    for i, n in enumerate(NS):
        for j, k in enumerate(KS):
            odd = (i + j) % 2 == 1
            groups.append(gr.D(rows, n, k, ldx_pad=1 if odd else 0, x_off=1 if odd else 0, db=db, w0=odd, ldw_pad=3 if odd else 0,
                               ldy_pad=2 if odd else 0))
    ops = gr.build_dw(gr.Case('dw', groups, seed=rows + (7 if db else 0)))
    arr, ws, bs, keep = _upload(ops)
    assert _call(built_lib, arr, len(ops)) == 0, built_lib.mg_last_error()
    fails = gr.check_dw(ops, [w.cpu() for w in ws], [b.cpu() if b is not None else None for b in bs])
    assert not fails, fails[:5]


@pytest.mark.parametrize('rows', [4099, 70000])
def test_five_calls_give_the_same_bits(built_lib, rows):
    ops = gr.build_dw(gr.Case('dw', [gr.D(rows, 128, 128, db=True, w0=True)], seed=11))
    first = None
    for _ in range(5):
        arr, ws, bs, keep = _upload(ops)
        assert _call(built_lib, arr, 1) == 0, built_lib.mg_last_error()
        got = (_bits(ws[0]), _bits(bs[0]))
        if first is None:
            first = got
            assert not torch.equal(first[0], _bits(ops[0]['dW'].cuda()))  # (something was added)
        assert torch.equal(got[0], first[0]) and torch.equal(got[1], first[1])


@pytest.mark.parametrize('target', [gr.D(420, 20, 57, db=True, w0=True), gr.D(4500, 129, 31, db=True, w0=True, ldx_pad=1, x_off=1)],
                         ids=['n20', 'n129'])
def test_a_group_does_not_depend_on_its_company(built_lib, target):
    """alone == among five others (wider ones, so the launch is compiled for another tile height) == in a call of more than DW_MAXG
    groups == with a scratch that holds little more than the largest group (the call is cut into many launches)"""
    others = [gr.D(140, 128, 64, db=True), gr.D(15, 3, 2), gr.D(65, 33, 128, w0=True), gr.D(420, 129, 31, db=True), gr.D(1, 1, 2)]
    many = [gr.D(15 + (i % 3), 3, 2 + (i % 2), db=i % 2 == 0) for i in range(70)]
    results = []
    for groups, at in (([target], 0), (others[:2] + [target] + others[2:], 2), (many[:40] + [target] + many[40:], 40)):
        ops = gr.build_dw(gr.Case('dw', groups, seed=3))
        ops[at] = gr.build_dw(gr.Case('dw', [target], seed=99))[0]  # the SAME operands for the target in every company
        for tight in (False, True):
            arr, ws, bs, keep = _upload(ops)
            nbytes = None
            if tight:
                from molgym_amd import _lib
                need, largest = C.c_size_t(0), 0
                for j in range(len(ops)):  # (the target is not the largest group of every company)
                    one = (_lib.GemmDwGroup * 1).from_buffer(arr, j * C.sizeof(_lib.GemmDwGroup))
                    assert built_lib.mg_gemm_dw_ordered_scratch_bytes(one, 1, C.byref(need)) == 0
                    largest = max(largest, need.value)
                nbytes = largest + 4096
            assert _call(built_lib, arr, len(ops), scratch_bytes=nbytes) == 0, built_lib.mg_last_error()
            results.append((_bits(ws[at]), _bits(bs[at])))
            if len(groups) > 1 and not tight:
                fails = gr.check_dw(ops, [w.cpu() for w in ws], [b.cpu() if b is not None else None for b in bs])
                assert not fails, fails[:5]
    for w, b in results[1:]:
        assert torch.equal(w, results[0][0]) and torch.equal(b, results[0][1])


def test_shared_destination_equals_successive_calls(built_lib):
    """two groups that add into the same dW / db (both uses of phi_beta in the agent): one call == two calls in list order"""
    a, b = gr.D(300, 33, 57, db=True, w0=True), gr.D(77, 33, 57, db=True, w0=True)
    ops = gr.build_dw(gr.Case('dw', [a, gr.D(15, 3, 2), b], seed=5))
    arr, ws, bs, keep = _upload(ops, share={2: 0})
    before = _bits(ws[0])
    assert _call(built_lib, arr, 3) == 0, built_lib.mg_last_error()
    together = (_bits(ws[0]), _bits(bs[0]))
    arr, ws, bs, keep = _upload(ops, share={2: 0})
    assert _call(built_lib, arr, 1, first=0) == 0, built_lib.mg_last_error()
    after_first = _bits(ws[0])
    assert _call(built_lib, arr, 1, first=2) == 0, built_lib.mg_last_error()
    assert not torch.equal(before, after_first) and not torch.equal(after_first, _bits(ws[0]))
    assert torch.equal(together[0], _bits(ws[0])) and torch.equal(together[1], _bits(bs[0]))
    # and the sum is the right one: the first group's reference with the second group's product on top
    w0, e0, b0, eb0 = gr.reference_dw(ops[0])
    w2, e2, b2, eb2 = gr.reference_dw(ops[2])
    o = ops[0]
    got = ws[0].cpu()[o['w_base']:o['w_base'] + 33 * o['ldw']].view(33, o['ldw'])[:, :57].double()
    want = w0 + (w2 - ops[2]['w_old'].double())
    assert bool(((got - want).abs() <= e0 + e2).all())


def test_concatenated_input_is_refused(built_lib):
    ops = gr.build_dw(gr.Case('dw', [gr.D(140, 32, 64, cat=(16, 40))], seed=1))
    arr, ws, bs, keep = _upload(ops)
    before = _bits(ws[0])
    assert _call(built_lib, arr, 1) == MG_EINVAL
    nbytes = C.c_size_t(1 << 20)
    scratch = torch.zeros(1 << 18, dtype=torch.float32, device='cuda')
    rc = built_lib.mg_test_gemm_dw_ordered(arr, 1, _ptr(scratch), nbytes, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == MG_EINVAL and torch.equal(before, _bits(ws[0]))


def test_default_dispatcher_never_takes_the_ordered_form(built_lib):
    """switch off: mg_test_gemm_dw launches forms of the GEMM_FORMS table only (the ordered form has no bit; a call that took it
    would report no form at all)"""
    from molgym_amd import _lib
    assert not _lib.is_deterministic()
    known = 0
    for bit in _lib.GEMM_FORMS.values():
        known |= 1 << bit
    for groups in ([gr.D(140, 32, 64, db=True)], [gr.D(420, 128, 128)], [gr.D(64, 129, 57, db=True), gr.D(15, 3, 2)]):
        ops = gr.build_dw(gr.Case('dw', groups, seed=2))
        arr, ws, bs, keep = _upload(ops)
        mask = C.c_uint64(0)
        rc = built_lib.mg_test_gemm_dw(arr, len(ops), C.byref(mask), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert rc == 0 and mask.value != 0 and mask.value & ~known == 0, (rc, hex(mask.value))
