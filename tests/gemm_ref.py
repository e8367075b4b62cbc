"""Float64 reference, derived error bound, guard checking and case list for the grouped GEMM dispatchers
(csrc/gemm_dispatch.inc: launch_gemm, launch_dw; reached through mg_test_gemm / mg_test_gemm_dw and their plan-only forms,
include/molgym_hip.h).

Used by tests/test_gemm_reference_host.py (no GPU: proves the comparator notices subtle errors), tests/test_gemm_plan_host.py (no
GPU: the planners alone over the whole sweep) and tests/test_gpu_gemm.py.
Everything here is CPU torch; the GPU test only uploads the operands, calls the library and hands the outputs back.
"""
import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

U = 2.0 ** -24           # unit roundoff of float32
LN2 = math.log(2.0)
SENTINEL = 0x7FA5C3D2    # bit pattern of every float the kernels must not write (a NaN, compared as int32)
GUARD_ROWS = 3           # rows of sentinels before and after every output
SLACK = 64               # floats after every operand (the weight-gradient forms over-read dY by < 32 floats)


def pick_nt(n):
    """column tile of the VALU forms (csrc/state.inc::pick_nt); ldm is N padded to it"""
    return 32 if n % 32 == 0 else 24 if n % 24 == 0 else 20 if n % 20 == 0 else 8


def pad_to(n, m):
    return (n + m - 1) // m * m


@dataclass
class G:
    """one group of a launch_gemm call"""
    rows: int
    N: int
    R: int
    nseg: int = 1
    ldx_pad: Tuple[int, ...] = (0, )   # ldx[s] = R + ldx_pad[s % len]
    x_off: int = 0                     # X[s] starts this many floats past a 16-byte boundary
    ldm_extra: int = 0                 # ldm = pad_to(N, pick_nt(N)) + ldm_extra (multiple of 4)
    ldy: Optional[int] = None          # default: N rounded up to 4, plus 4 (at least four pad columns)
    y_off: int = 0                     # Y starts this many floats past a 16-byte boundary
    bias: bool = False
    act: int = 0                       # 0 none, 1 ReLU, 2 softplus - ln 2
    mask: int = 0                      # posmask mode 0 (none), 1, 2
    rowscale: bool = False
    resid: bool = False
    acc: bool = False


@dataclass
class D:
    """one group of a launch_dw call"""
    rows: int
    N: int
    K: int
    ldx_pad: int = 0
    x_off: int = 0                     # floats past a 16-byte boundary (1: 4 bytes, 2: 8 bytes)
    cat: Optional[Tuple[int, int]] = None   # (ks1, ks2): columns [ks1, ks2) from X1, [ks2, K) from X2
    db: bool = False
    w0: bool = False                   # dW (and db) start non-zero
    ldw_pad: int = 0
    ldy_pad: int = 0


@dataclass
class Case:
    kind: str                          # 'gemm' or 'dw'
    groups: list
    seed: int = 0
    forms: Optional[frozenset] = None  # forms the DEFAULT switches must launch for this call (None: not asserted per case)
    einval_in: Tuple[str, ...] = ()    # profiles in which the dispatcher must refuse the call with MG_EINVAL
    name: str = ''

    def label(self):
        return self.name or f'{self.kind} seed {self.seed}: ' + '; '.join(str(g) for g in self.groups)


# ---- operands ------------------------------------------------------------------------------------------------------
_POOL = None


def _randn(n, gen):
    """n seeded N(0, 1) float32; large requests are cut from one pool at a seeded offset (drawing 50 M normals per case costs
    more than the product under test)"""
    global _POOL
    if gen is None:   # layout only (build_gemm / build_dw with fill=False): the contents are never read
        return torch.empty(n, dtype=torch.float32)
    if n <= (1 << 16):
        return torch.randn(n, generator=gen, dtype=torch.float32)
    if _POOL is None:
        _POOL = torch.randn(1 << 24, generator=torch.Generator().manual_seed(12345), dtype=torch.float32)
    off = int(torch.randint(0, _POOL.numel(), (1, ), generator=gen))
    reps = (off + n + _POOL.numel() - 1) // _POOL.numel()
    src = _POOL if reps == 1 else _POOL.repeat(reps)
    return src[off:off + n].clone()


def _sentinel(n, gen=True):
    if gen is None:
        return torch.empty(n, dtype=torch.float32)
    return torch.full((n, ), SENTINEL, dtype=torch.int32).view(torch.float32)


def _matrix(rows, cols, ld, off, gen, pad_value):
    """a [rows][cols] N(0, 1) matrix of pitch ld inside its own flat buffer, starting `off` floats in; pad columns = pad_value"""
    if gen is None:
        flat = torch.empty(off + rows * ld + SLACK, dtype=torch.float32)
        return flat, flat[off:off + rows * ld].view(rows, ld)
    flat = torch.full((off + rows * ld + SLACK, ), float(pad_value), dtype=torch.float32)
    view = flat[off:off + rows * ld].view(rows, ld)
    view[:, :cols] = _randn(rows * cols, gen).view(rows, cols)
    return flat, view


def _special_rows(rows):
    """(row of exact zeros, row of ones with one 1e4) or (None, None): a wrong row index or a dropped large term cannot hide"""
    if rows < 3:
        return None, None
    return rows // 3, (2 * rows) // 3


def _output(rows, cols, ld, off, gen, fill):
    """an output [rows][cols] of pitch ld with GUARD_ROWS sentinel rows on both sides and sentinel pad columns; the interior holds
    `fill` ('randn' or 'zeros').  Returns (flat buffer, offset of element [0][0] in floats, interior view)"""
    total = (rows + 2 * GUARD_ROWS) * ld
    flat = _sentinel(off + total + SLACK, gen)
    base = off + GUARD_ROWS * ld
    view = flat[base:base + rows * ld].view(rows, ld)
    if gen is not None:
        view[:, :cols] = _randn(rows * cols, gen).view(rows, cols) if fill == 'randn' else 0.0
    return flat, base, view


def build_gemm(case, fill=True):
    """CPU operands of a launch_gemm case: a list (one per group) of dicts of flat float32 buffers + views + layout.
    fill=False: the same buffers, sizes and offsets with their contents left uninitialised (the planners look at the layout only)"""
    gen = torch.Generator().manual_seed(1000 + case.seed) if fill else None
    out = []
    for g in case.groups:
        o = {'g': g, 'ldm': pad_to(g.N, pick_nt(g.N)) + g.ldm_extra, 'ldy': g.ldy if g.ldy is not None else pad_to(g.N, 4) + 4}
        assert o['ldy'] >= g.N and o['ldm'] % 4 == 0
        zr, br = _special_rows(g.rows) if fill else (None, None)
        o['X'], o['M'], o['ldx'] = [], [], []
        for s in range(g.nseg):
            ldx = g.R + g.ldx_pad[s % len(g.ldx_pad)]
            flat, view = _matrix(g.rows, g.R, ldx, g.x_off, gen, 1e4)   # a pad column that is read shows as an error of 1e4
            if zr is not None:
                view[zr, :g.R] = 0.0
                view[br, :g.R] = 1.0
                if s == 0:
                    view[br, g.R // 2] = 1e4
            mflat, _ = _matrix(g.R, g.N, o['ldm'], 0, gen, 0.0)          # zero padded to ldm (precondition)
            if fill:
                mflat[g.R * o['ldm']:] = 1e4                             # a reduction that runs past row R meets this, not zeros
            o['X'].append((flat, view)); o['M'].append((mflat, mflat[:g.R * o['ldm']].view(g.R, o['ldm']))); o['ldx'].append(ldx)
        o['bias'] = _randn(g.N, gen) if g.bias else None
        o['rowscale'] = _randn(g.rows, gen) if g.rowscale else None
        o['mask'] = _matrix(g.rows, g.N, g.N + 3, 0, gen, 1e4) if g.mask else None
        o['resid'] = _matrix(g.rows, g.N, g.N + 1, 0, gen, 1e4) if g.resid else None
        o['Y'], o['y_base'], yview = _output(g.rows, g.N, o['ldy'], g.y_off, gen, 'randn')
        o['y_old'] = yview[:, :g.N].clone() if fill else None
        out.append(o)
    return out


def build_dw(case, fill=True):
    gen = torch.Generator().manual_seed(5000 + case.seed) if fill else None
    out = []
    for d in case.groups:
        o = {'g': d, 'ldy': d.N + d.ldy_pad, 'ldw': d.K + d.ldw_pad}
        zr, br = _special_rows(d.rows) if fill else (None, None)
        o['dY'] = _matrix(d.rows, d.N, o['ldy'], 0, gen, 1e4)
        bounds = [0, d.K] if d.cat is None else [0, d.cat[0], d.cat[1], d.K]
        o['X'] = []
        for s in range(len(bounds) - 1):
            w = bounds[s + 1] - bounds[s]
            ld = w + d.ldx_pad
            o['X'].append(_matrix(d.rows, w, ld, d.x_off if s == 0 else 0, gen, 1e4) + (ld, ))
        if zr is not None:
            for _, v, _ in o['X']:
                v[zr, :] = 0.0
            o['dY'][1][br, :d.N] = 1.0
            o['dY'][1][br, d.N // 2] = 1e4
            # and one in the LAST row: at >= 65536 rows the worst-case bound is 0.4 % of S, so a lost tail chunk of N(0, 1) rows
            # would pass; a lost 1e4 does not
            o['dY'][1][d.rows - 1, :d.N] = 1.0
            o['dY'][1][d.rows - 1, d.N // 3] = 1e4
        o['dW'], o['w_base'], wview = _output(d.N, d.K, o['ldw'], 0, gen, 'randn' if d.w0 else 'zeros')
        o['w_old'] = wview[:, :d.K].clone()
        o['db'] = None
        if d.db:
            o['db'], o['b_base'], bview = _output(1, d.N, d.N + 4, 0, gen, 'randn' if d.w0 else 'zeros')
            o['b_old'] = bview[0, :d.N].clone()
        out.append(o)
    return out


# ---- descriptors -----------------------------------------------------------------------------------------------------------
def _ptr(t, off=0):
    return C.c_void_p(t.data_ptr() + 4 * off)


def gemm_groups(ops, place=lambda t: t):
    """the mg_gemm_group array of build_gemm operands.  place(tensor) -> the tensor whose address goes into the descriptor: the GPU
    test uploads (and keeps the copy alive), the host test hands the CPU buffers themselves -- the planners look at alignment only.
    Returns (array, the placed Y buffers)"""
    from molgym_amd import _lib
    arr, ys = (_lib.GemmGroup * len(ops))(), []
    for a, o in zip(arr, ops):
        g = o['g']
        for s in range(g.nseg):
            a.X[s] = _ptr(place(o['X'][s][0]), g.x_off).value
            a.M[s] = _ptr(place(o['M'][s][0])).value
            a.ldx[s] = o['ldx'][s]
        a.nseg = g.nseg
        a.bias = _ptr(place(o['bias'])) if g.bias else None
        a.rowscale = _ptr(place(o['rowscale'])) if g.rowscale else None
        if g.mask:
            a.posmask, a.ld_mask, a.mask_mode = _ptr(place(o['mask'][0])), g.N + 3, g.mask
        if g.resid:
            a.resid, a.ld_resid = _ptr(place(o['resid'][0])), g.N + 1
        ys.append(place(o['Y']))
        a.Y = _ptr(ys[-1], o['y_base'])
        a.ldm, a.ldy, a.R, a.N, a.rows, a.relu, a.accumulate = o['ldm'], o['ldy'], g.R, g.N, g.rows, g.act, int(g.acc)
    return arr, ys


def dw_groups(ops, place=lambda t: t):
    """the mg_gemm_dw_group array of build_dw operands (place: as gemm_groups).  Returns (array, placed dW buffers, placed db buffers)"""
    from molgym_amd import _lib
    arr, ws, bs = (_lib.GemmDwGroup * len(ops))(), [], []
    for a, o in zip(arr, ops):
        d = o['g']
        a.dY = _ptr(place(o['dY'][0]))
        a.X = _ptr(place(o['X'][0][0]), d.x_off)
        a.ldx = o['X'][0][2]
        if d.cat is not None:
            a.X1, a.ldx1, a.ks1 = _ptr(place(o['X'][1][0])), o['X'][1][2], d.cat[0]
            a.X2, a.ldx2, a.ks2 = _ptr(place(o['X'][2][0])), o['X'][2][2], d.cat[1]
        ws.append(place(o['dW']))
        a.dW = _ptr(ws[-1], o['w_base'])
        bs.append(place(o['db']) if d.db else None)
        a.db = _ptr(bs[-1], o['b_base']) if d.db else None
        a.ldy, a.ldw, a.N, a.K, a.rows = o['ldy'], o['ldw'], d.N, d.K, d.rows
    return arr, ws, bs


# ---- reference and bound -------------------------------------------------------------------------------------------
def _gamma(n):
    """(1 + u)^n - 1 <= n u / (1 - n u): the relative error of a value that went through at most n float32 roundings"""
    return n * U / (1.0 - n * U)


def reference_gemm(o):
    """float64 reference of one group and its per-element error bound.

    Reference: torch.matmul in float64 over exactly the float32 operands, then the epilogue of gemm_epilogue (csrc/gemm.inc) in
    float64 and in its order: bias, activation, posmask, rowscale, resid, accumulate.

    Bound, derived (no constant comes from what the kernels produce).  K = total reduction length over the segments,
    S = |X| @ |M| + |bias|, u = 2^-24:
      * pre-activation v: every term of the sum goes through one rounding of its product (none with FMA / the MFMA's exact
        products) and at most K additions (K products plus the bias are K + 1 terms), i.e. at most K + 1 roundings WHATEVER the
        order -- lanes, waves, LDS combines or atomics.  e = gamma(K + 4) S with gamma(n) = n u / (1 - n u); the + 3 are three
        spare roundings (a combine through float32 LDS partial sums re-rounds nothing new, but this keeps the bound independent of
        how a form splits the sum);
      * activation: ReLU and softplus are 1-Lipschitz, so e carries over; softplus - ln 2 is evaluated with float32 expf, log1pf
        (each within 2 ulp of a value <= |a| + ln 2 + 1) and one subtraction: + 8 u (|a| + 1);
      * posmask mode 1 keeps or zeroes (exact); mode 2 multiplies by f = 1 - 0.5 exp(-mask), itself within 4 u (|f| + 1) (expf,
        one product, one subtraction): e <- |f| e + 4 u (|f| + 1) |a| + u |a f|;
      * rowscale, resid, accumulate: one rounding each of the magnitude they produce, doubled (the kernel rounds its own value,
        not the reference's): e <- |rs| e + 2 u |y|;  e <- e + 2 u |y| after each of the two additions.
    Without flags this is gamma(K + 4) S; with all of them it stays below |rs| |f| gamma(K + 4) S + 8 u (|y| + |resid| + |y_old| + 1)
    times small factors of |rs| (|f| + 1).
    """
    g = o['g']
    K = g.R * g.nseg
    v = torch.zeros(g.rows, g.N, dtype=torch.float64)
    S = torch.zeros(g.rows, g.N, dtype=torch.float64)
    for (_, x), (_, m) in zip(o['X'], o['M']):
        xd, md = x[:, :g.R].double(), m[:, :g.N].double()
        v += xd @ md
        S += xd.abs() @ md.abs()
    if o['bias'] is not None:
        v += o['bias'].double()
        S += o['bias'].double().abs()
    e = S.mul_(_gamma(K + 4))
    if g.act == 1:
        v = v.clamp_(min=0.0)
    elif g.act == 2:
        v = torch.nn.functional.softplus(v, beta=1.0, threshold=40.0).sub_(LN2)
        e += 8 * U * (v.abs() + 1.0)
    if o['mask'] is not None:
        a = o['mask'][1][:, :g.N].double()
        if g.mask == 2:
            f = 1.0 - 0.5 * torch.exp(-a)
            e = f.abs() * e + 4 * U * (f.abs() + 1.0) * v.abs() + U * (v * f).abs()
            v = v * f
        else:
            keep = a > 0
            v = torch.where(keep, v, torch.zeros_like(v))
            e = torch.where(keep, e, torch.zeros_like(e))
    if o['rowscale'] is not None:
        rs = o['rowscale'].double()[:, None]
        v = v * rs
        e = e * rs.abs() + 2 * U * v.abs()
    if o['resid'] is not None:
        v = v + o['resid'][1][:, :g.N].double()
        e = e + 2 * U * v.abs()
    if g.acc:
        v = v + o['y_old'].double()
        e = e + 2 * U * v.abs()
    return v, e


def _dw_x(o):
    d = o['g']
    return torch.cat([v[:, :w - d.ldx_pad] for _, v, w in o['X']], dim=1)


def reference_dw(o):
    """float64 reference of one weight-gradient group: dW = dW_old + dY^T X, db = db_old + column sums of dY, and their bounds.

    The reduction runs over the rows; the kernels add partial tiles with float32 atomics in an arbitrary order, on top of the
    previous contents: each term goes through at most rows + 1 additions whatever the order, so with S = |dY|^T |X| + |dW_old|
    the error is at most gamma(rows + 4) S (see reference_gemm for gamma and the spare roundings); the bias gradient is the same
    sum with X = 1."""
    d = o['g']
    yd = o['dY'][1][:, :d.N].double()
    xd = _dw_x(o).double()
    w = o['w_old'].double() + yd.t() @ xd
    ew = (o['w_old'].double().abs() + yd.abs().t() @ xd.abs()) * _gamma(d.rows + 4)
    b = eb = None
    if o['db'] is not None:
        b = o['b_old'].double() + yd.sum(0)
        eb = (o['b_old'].double().abs() + yd.abs().sum(0)) * _gamma(d.rows + 4)
    return w, ew, b, eb


# ---- comparison ----------------------------------------------------------------------------------------------------
# No kernel is documented to write outside [rows][0..N), so there is no exemption: every float around the interior must come back
# bit-identical.
def _check_output(flat_before, flat_after, base, rows, cols, ld, ref, bound, what):
    """failures (strings) of one output: interior against ref within bound, everything else bit-identical to before"""
    fails = []
    before, after = flat_before.view(torch.int32), flat_after.view(torch.int32)
    end = base + rows * ld
    # the three regions around the interior: everything in front (guard rows), the pad columns, everything behind
    pads = before[base:end].view(rows, ld)[:, cols:] != after[base:end].view(rows, ld)[:, cols:]
    head, tail = before[:base] != after[:base], before[end:] != after[end:]
    nchanged = int(head.sum()) + int(pads.sum()) + int(tail.sum())
    if nchanged:
        if bool(head.any()):
            r, c = divmod(int(head.nonzero()[0]) - base, ld)
        elif bool(pads.any()):
            r, c = (int(v) for v in pads.nonzero()[0])
            c += cols
        else:
            r, c = divmod(int(tail.nonzero()[0]) + rows * ld, ld)
        fails.append(f'{what}: {nchanged} floats outside [rows][N) were written, first at row {r} column {c} (pitch {ld})')
    got = flat_after[base:end].view(rows, ld)[:, :cols].double()
    err = (got - ref).abs_()
    bad = ~(err <= bound)   # NaN compares false: a sentinel left in the interior fails
    if bool(bad.any()):
        idx = int(bad.flatten().nonzero()[0])
        r, c = divmod(idx, cols)
        ratio = torch.where(bound > 0, err / bound, err * float('inf')).nan_to_num(nan=float('inf'))[bad]
        fails.append(f'{what}: {int(bad.sum())} of {rows * cols} entries out of bound, first at [{r}][{c}]: got {got[r, c].item()!r} '
                     f'want {ref[r, c].item()!r} bound {bound[r, c].item():.3e} (worst error / bound {ratio.max().item():.3g})')
    return fails


def check_gemm(ops, ys_after):
    """ops: build_gemm(case); ys_after: the flat Y buffers after the call (CPU).  Returns the list of failures."""
    fails = []
    for i, (o, y) in enumerate(zip(ops, ys_after)):
        g = o['g']
        ref, bound = reference_gemm(o)
        fails += _check_output(o['Y'], y, o['y_base'], g.rows, g.N, o['ldy'], ref, bound, f'group {i} Y')
    return fails


def check_dw(ops, ws_after, bs_after):
    fails = []
    for i, (o, w, b) in enumerate(zip(ops, ws_after, bs_after)):
        d = o['g']
        rw, ew, rb, eb = reference_dw(o)
        fails += _check_output(o['dW'], w, o['w_base'], d.N, d.K, o['ldw'], rw, ew, f'group {i} dW')
        if o['db'] is not None:
            fails += _check_output(o['db'], b, o['b_base'], 1, d.N, d.N + 4, rb[None, :], eb[None, :], f'group {i} db')
    return fails


# ---- an honest float32 "kernel" on the CPU (tests/test_gemm_reference_host.py) -------------------------------------------
def float32_gemm(o, corrupt=None):
    """what a correct float32 kernel computes, written into a copy of the Y buffer; `corrupt` names one deliberate defect"""
    g = o['g']
    xs = [x[:, :g.R] for _, x in o['X']]
    ms = [m[:, :g.N] for _, m in o['M']]
    if corrupt == 'bf16':
        xs = [x.bfloat16().float() for x in xs]
        ms = [m.bfloat16().float() for m in ms]
    if corrupt == 'drop_k':   # one reduction index omitted
        xs = [xs[0].clone()] + xs[1:]
        xs[0][:, g.R // 3] = 0.0
    v = torch.zeros(g.rows, g.N, dtype=torch.float32)
    for x, m in zip(xs, ms):
        v += x @ m
    if corrupt == 'tile_shift':   # the second 16-row tile computed from the first tile's rows
        n = min(32, g.rows) - 16
        v[16:16 + n] = v[0:n].clone()
    if o['bias'] is not None:
        v += o['bias']
    if g.act == 1:
        v = v.clamp(min=0.0)
    elif g.act == 2:
        v = torch.where(v > 20.0, v, torch.log1p(torch.exp(v))) - torch.tensor(LN2, dtype=torch.float32)
    if o['mask'] is not None:
        a = o['mask'][1][:, :g.N]
        v = v * (1.0 - 0.5 * torch.exp(-a)) if g.mask == 2 else torch.where(a > 0, v, torch.zeros_like(v))
    if o['rowscale'] is not None:
        v = v * o['rowscale'][:, None]
    if o['resid'] is not None:
        v = v + o['resid'][1][:, :g.N]
    if g.acc and corrupt != 'no_acc':
        v = v + o['y_old']
    y = o['Y'].clone()
    view = y[o['y_base']:o['y_base'] + g.rows * o['ldy']].view(g.rows, o['ldy'])
    if corrupt == 'tail_cols' and g.N % 4:   # the last N % 4 columns left at their previous contents
        view[:, :g.N - g.N % 4] = v[:, :g.N - g.N % 4]
    else:
        view[:, :g.N] = v
    if corrupt == 'pad_write':
        view[g.rows // 2, g.N] = v[g.rows // 2, g.N - 1]
    return y


def float32_dw(o):
    d = o['g']
    w = o['dW'].clone()
    view = w[o['w_base']:o['w_base'] + d.N * o['ldw']].view(d.N, o['ldw'])
    view[:, :d.K] = o['w_old'] + o['dY'][1][:, :d.N].t() @ _dw_x(o)
    b = None
    if o['db'] is not None:
        b = o['db'].clone()
        b[o['b_base']:o['b_base'] + d.N] = o['b_old'] + o['dY'][1][:, :d.N].sum(0)
    return w, b


# ---- the sweep -------------------------------------------------------------------------------------------------------
# Derived from the planners' conditions (csrc/gemm_dispatch.inc: plan_gemm, plan_gemm_dw; DESIGN.md "GEMM forms" has the same
# table).  tests/test_gemm_plan_host.py checks this statement against the planners without a GPU.
#   plan_gemm, in this order
#     col_form = one segment, one R for all groups, R % 4 == 0, 8 <= R <= 64, every N > 32
#     rows_unaligned   some R % 4 / ldx % 4 / X not 16-byte aligned, max N <= 128, not col_form
#     rows_ws          rows >= 16384, every R >= 128, one segment, max N <= 48, every N % 4 == 0, weights <= 80 KB of LDS
#     rows64_rt2       rows >= 16384, max N <= 48, every R >= 8 (two 16-row tiles per wave)
#     rows_w16         max N <= 48, some R >= 160, row tiles x groups <= 4096
#     rows_w4          max N <= 128, every R >= 8
#     -- from here one launch per group when the groups' column tiles (pick_nt) differ --
#     cols_ws          col_form, R in {20, 24, 40}, no bias / activation / mask / resid, ldy % 4 == 0, Y aligned, N <= 704
#     mfma_cols_exact  col_form, R in {8, 20, 24, 40};  mfma_cols_generic: the other R
#     rows_lds         aligned, every R >= 16, rows >= 8192
#     valu_rows        the rest (R = 4; N > 128 with R > 64 at small row counts; unaligned with N > 128)
#   plan_gemm_dw (per run of one class: N <= 32, <= 48, <= 128, VALU tiles)
#     dw4              max N <= 48, max K >= 64, rows >= 65536, every K % 4 == 0, ldx % 4 == 0, X 16-byte aligned
#     dw2              max N <= 48, max K >= 32, every K and ldx even, X 8-byte aligned
#     dw               N <= 128;   valu_dw: N > 128 (or MG_MFMA_DW=0)
ROWS = (1, 15, 16, 17, 63, 64, 65, 140, 420, 16383, 16384, 16400)
ROW_N = (1, 3, 16, 17, 20, 32, 33, 40, 48, 49, 64, 100, 128)
ROW_R = (8, 12, 56, 128, 160, 220, 700)
COL_R = (8, 20, 24, 40, 12, 32, 48, 64)
COL_N = (33, 34, 48, 62, 64, 220, 222, 700, 704, 708)
COL_ROWS = (5, 16, 140, 420, 40000)
DW_N = (1, 20, 32, 33, 40, 48, 49, 128, 129, 256)
DW_K = (2, 31, 32, 56, 64, 220, 700, 57)
DW_ROWS = (1, 15, 64, 140, 420, 65535, 65536, 70000)
FLAGS = ('bias', 'relu', 'softplus', 'mask1', 'mask2', 'rowscale', 'resid', 'acc', 'all')
PROFILES = {
    'default': {},
    # the VALU fallbacks
    'valu': dict(MG_MFMA='0', MG_MFMA_DX='0', MG_MFMA_DW='0'),
    # the same forms at other geometry: several row tiles per cols_ws workgroup, and the 16-byte weight-gradient form at every row
    # count -- at >= 65536 rows, where the default takes it, the worst-case bound is wide; at 140 rows it is tight
    'alt': dict(MG_COLS_WS_WGS='64', MG_DW4_MINROWS='1'),
}


def _flags(name):
    return {
        'plain': {}, 'bias': dict(bias=True), 'relu': dict(bias=True, act=1), 'softplus': dict(bias=True, act=2),
        'mask1': dict(mask=1), 'mask2': dict(mask=2), 'rowscale': dict(rowscale=True), 'resid': dict(resid=True),
        'acc': dict(acc=True), 'all': dict(bias=True, act=2, mask=2, rowscale=True, resid=True, acc=True),
        'all_relu': dict(bias=True, act=1, mask=1, rowscale=True, resid=True, acc=True),
    }[name]


def F(*names):
    return frozenset(names)


def blocks():
    """name -> list of Case.  The same list for every profile (the switches change which form a shape reaches, not the shapes)."""
    b = {}
    seed = [0]

    def case(kind, groups, **kw):
        seed[0] += 1
        return Case(kind, list(groups), seed=seed[0], **kw)

    # -- row forms: the full cross of row counts, widths and reduction lengths, one group per call
    for rows in ROWS:
        for R in ROW_R:
            b[f'rows_{rows}_R{R}'] = [case('gemm', [G(rows, N, R)]) for N in ROW_N]
    # -- segments (one to five, different pitches), every epilogue flag alone and all together, at the edges of the row tiles
    b['segments'] = [case('gemm', [G(rows, N, R, nseg=ns, ldx_pad=(0, 4, 12, 8, 20))])
                     for ns in (1, 2, 3, 4, 5) for rows, N, R in ((17, 20, 56), (140, 33, 220), (65, 48, 160), (16400, 20, 128), (420, 100, 12))]
    b['flags'] = [case('gemm', [G(rows, N, R, **_flags(f))]) for f in FLAGS + ('all_relu', )
                  for rows, N, R in ((65, 20, 56), (140, 33, 220), (63, 128, 128), (17, 3, 12))]
    b['flags_large'] = [case('gemm', [G(rows, N, R, **_flags(f))]) for f in ('softplus', 'all', 'all_relu', 'acc')
                        for rows, N, R in ((16400, 20, 220), (16384, 40, 56), (16383, 33, 128))]
    b['pitches'] = [case('gemm', [G(rows, N, R, ldx_pad=(8, ), ldm_extra=8, ldy=N + 5, y_off=1, **_flags('all'))])
                    for rows, N, R in ((65, 20, 56), (140, 17, 220), (16400, 20, 128), (16, 64, 8))]
    # -- several groups of mixed R / N in one call, and more than GEMM_MAXG = 16 groups (the recursive split)
    mixed = [G(140, 20, 56), G(15, 3, 8, bias=True), G(65, 32, 220, act=1, bias=True), G(1, 17, 128), G(420, 48, 700, acc=True),
             G(64, 33, 12, rowscale=True)]
    b['groups'] = [
        case('gemm', mixed, forms=F('rows_w16')),
        case('gemm', [G(63 + 7 * i, (1, 3, 16, 17, 20, 32, 33)[i % 7], (8, 12, 56, 128)[i % 4], bias=bool(i & 1)) for i in range(19)],
             forms=F('rows_w4')),
        case('gemm', [G(140, 64, 56), G(17, 128, 128, resid=True), G(16, 100, 8)], forms=F('rows_w4')),
        case('gemm', [G(140, 20, 56), G(0, 20, 56), G(17, 20, 56)]),   # an empty group is skipped
        case('gemm', [G(16400, 20, 220), G(16384, 20, 700), G(140, 16, 128)], forms=F('rows_ws')),
        case('gemm', [G(16400, 20, 56), G(420, 33, 220, nseg=2)], forms=F('rows64_rt2')),
        # N > 128 with mixed column tiles: one launch per group -- R <= 64 is a column shape on its own, R = 220 / 72 are not
        case('gemm', [G(140, 160, 56), G(17, 136, 12), G(65, 144, 220)], forms=F('mfma_cols_generic', 'valu_rows')),
        case('gemm', [G(140, 160, 72), G(17, 136, 220), G(65, 144, 4)], forms=F('valu_rows')),
    ]
    # -- the guarded form: R % 4 != 0, ldx % 4 != 0, X offset by one float
    b['unaligned'] = [case('gemm', [g], forms=F('rows_unaligned')) for g in (
        G(140, 20, 25), G(17, 33, 3), G(65, 128, 57), G(1, 1, 1), G(16400, 20, 25), G(140, 48, 220, ldx_pad=(1, )), G(63, 17, 56, x_off=1),
        G(16384, 40, 128, x_off=1), G(140, 20, 221, nseg=3, ldx_pad=(3, 0, 1)), G(64, 100, 30, **_flags('all')))]
    b['unaligned'] += [case('gemm', [G(140, 20, 56), G(17, 16, 25)], forms=F('rows_unaligned')),   # one odd group sends the whole call there
                       case('gemm', [G(140, 160, 25)], forms=F('valu_rows')), case('gemm', [G(140, 130, 72, x_off=1)], forms=F('valu_rows')),
                       case('gemm', [G(140, 130, 56, x_off=1)], forms=F('mfma_cols_generic')),
                       # a misaligned X in column shape stays with the column forms (dword loads)
                       case('gemm', [G(140, 222, 20, x_off=1)], forms=F('cols_ws')), case('gemm', [G(140, 100, 8, x_off=1)], forms=F('mfma_cols_exact'))]
    # -- LDS-stationary weights: each rows_ws_ldw class, both sides of the 80 KB LDS limit
    ws = [case('gemm', [G(rows, N, R)], forms=F('rows_ws')) for N in (4, 20, 24, 28, 32, 36, 44, 48) for rows, R in ((16384, 128), (16400, 220))]
    ws += [case('gemm', [G(16400, 20, 700)], forms=F('rows_ws')),
           case('gemm', [G(16400, 28, 704)], forms=F('rows_ws')),        # 704 x 28 x 4 = 78848 bytes: just under 80 KB
           case('gemm', [G(16400, 28, 768)], forms=F('rows64_rt2')),     # 86016: just over
           case('gemm', [G(16400, 48, 384)], forms=F('rows_ws')),        # 384 x 52 x 4 = 79872: just under
           case('gemm', [G(16400, 48, 448)], forms=F('rows64_rt2')),     # 93184: just over
           case('gemm', [G(16400, 48, 768)], forms=F('rows64_rt2')),     # 159744 = 156 KB exactly
           case('gemm', [G(16400, 48, 832)], forms=F('rows64_rt2')),     # 173056
           case('gemm', [G(16400, 36, 700)], forms=F('rows64_rt2')),     # 101376
           case('gemm', [G(16383, 20, 220)], forms=F('rows_w16')),       # one row short of the threshold
           case('gemm', [G(33000, 20, 220, **_flags('all'))], forms=F('rows_ws')),
           case('gemm', [G(16400, 44, 220, rowscale=True, acc=True)], forms=F('rows_ws'))]
    b['rows_ws'] = ws
    # -- rows64: the same row counts with R < 128 or N % 4 != 0
    b['rows64'] = [case('gemm', [G(rows, N, R)], forms=F('rows64_rt2')) for rows in (16384, 16400, 16511) for N, R in
                   ((20, 56), (33, 220), (32, 8), (1, 128), (17, 700), (40, 124), (48, 100), (30, 128))]
    # -- both operands through LDS: rows >= 8192, N > 128
    b['rows_lds'] = [case('gemm', [G(rows, N, R, **_flags(f))], forms=F('rows_lds')) for rows, N, R, f in (
        (8192, 160, 128, 'plain'), (8200, 129, 72, 'bias'), (8192, 256, 68, 'all'), (8255, 136, 220, 'relu'), (9000, 140, 72, 'acc'),
        (8192, 192, 128, 'plain'))]
    b['rows_lds'] += [case('gemm', [G(8191, 160, 128)], forms=F('valu_rows')), case('gemm', [G(8200, 160, 4)], forms=F('valu_rows')),
                      case('gemm', [G(8200, 160, 128, nseg=2, ldx_pad=(0, 4))], forms=F('rows_lds'))]
    # -- VALU forms reachable by default: R = 4, or N > 128 at small row counts
    b['valu_rows'] = [case('gemm', [G(rows, N, R, **_flags(f))], forms=F('valu_rows')) for rows, N, R, f in (
        (140, 20, 4, 'plain'), (17, 33, 4, 'bias'), (16400, 20, 4, 'plain'), (65, 128, 4, 'all'), (140, 129, 72, 'plain'), (17, 160, 128, 'relu'),
        (420, 256, 220, 'all'), (64, 136, 700, 'plain'), (1, 192, 4, 'plain'), (140, 144, 4, 'resid'), (5000, 130, 2, 'acc'))]
    # -- column forms: the full cross at the small row counts, plain / accumulate / rowscale / not plain
    for R in COL_R:
        for var in ('plain', 'acc', 'rowscale', 'bias', 'mask1'):
            b[f'cols_R{R}_{var}'] = [case('gemm', [G(rows, N, R, ldy=pad_to(N, 4) if N % 4 else None, **_flags(var))])
                                     for rows in COL_ROWS for N in COL_N]   # 40000 rows = 2500 row tiles: several per cols_ws workgroup
    b['cols_misc'] = [
        # THE regression case: the straight-line path of k_gemm_mfma_cols_ws dropped the partial last column quad
        case('gemm', [G(140, 222, 20, ldy=224)], forms=F('cols_ws'), name='cols_ws N % 4 != 0: R = 20, N = 222, ldy = 224, plain'),
        case('gemm', [G(40000, 222, 20, ldy=224)], forms=F('cols_ws')),                  # the same with several row tiles per workgroup
        case('gemm', [G(140, 222, 20, ldy=223)], forms=F('mfma_cols_exact')),            # ldy % 4 != 0: scalar epilogue
        case('gemm', [G(140, 220, 24, y_off=1)], forms=F('mfma_cols_exact')),            # Y not 16-byte aligned
        case('gemm', [G(140, 220, 20, resid=True)], forms=F('mfma_cols_exact')),
        case('gemm', [G(140, 220, 40, mask=2)], forms=F('mfma_cols_exact')),
        case('gemm', [G(140, 700, 20), G(420, 222, 20), G(5, 34, 20), G(16, 704, 20, acc=True)], forms=F('cols_ws')),
        case('gemm', [G(140, 700, 40), G(420, 62, 40, rowscale=True)], forms=F('cols_ws')),
        case('gemm', [G(140, 220, 12), G(17, 34, 12)], forms=F('mfma_cols_generic')),
        case('gemm', [G(140, 222, 64, **_flags('all'))], forms=F('mfma_cols_generic')),
        # a group of N <= 32 breaks the column shape of the call; N > 128 then splits it by column tile: one launch per group
        case('gemm', [G(140, 220, 20), G(140, 32, 20)], forms=F('cols_ws', 'rows_w4')),
        case('gemm', [G(140, 100, 20), G(140, 100, 24)], forms=F('rows_w4')),            # two R: not a column shape
    ]
    # -- weight gradients: the full cross of row counts, widths and reduction-side lengths, the bias gradient on for half of it
    for rows in DW_ROWS:
        for K in DW_K:
            b[f'dw_{rows}_K{K}'] = [case('dw', [D(rows, N, K, db=bool((N + K) & 1))]) for N in DW_N]
    # the variants on both sides of the dw4 threshold: db on where the cross has it off, dW starting non-zero, X misaligned
    b['dw_threshold'] = [case('dw', [D(rows, N, K, **kw)]) for rows in (65535, 70000) for N, K in ((20, 220), (48, 64), (33, 57), (129, 32))
                         for kw in (dict(db=not (N + K) & 1), dict(w0=True, db=True), dict(x_off=1), dict(x_off=2, w0=True))]
    b['dw_misc'] = [
        case('dw', [D(65536, 20, 220)], forms=F('dw4')), case('dw', [D(70000, 48, 64, db=True)], forms=F('dw4')),
        case('dw', [D(65535, 20, 220)], forms=F('dw2')), case('dw', [D(65536, 49, 220)], forms=F('dw')),
        case('dw', [D(65536, 20, 56)], forms=F('dw2')), case('dw', [D(65536, 20, 222)], forms=F('dw2')),
        case('dw', [D(140, 20, 31)], forms=F('dw')), case('dw', [D(140, 20, 57, db=True)], forms=F('dw')),
        case('dw', [D(140, 129, 56, db=True)], forms=F('valu_dw')), case('dw', [D(420, 256, 700, db=True, w0=True)], forms=F('valu_dw')),
        # X misaligned by 4 / 8 bytes
        case('dw', [D(420, 20, 56, x_off=1, db=True)], forms=F('dw')), case('dw', [D(420, 20, 56, x_off=2)], forms=F('dw2')),
        case('dw', [D(65536, 20, 64, x_off=2, db=True)], forms=F('dw2')), case('dw', [D(65536, 40, 64, x_off=1)], forms=F('dw')),
        case('dw', [D(140, 48, 220, ldx_pad=1)], forms=F('dw')), case('dw', [D(140, 48, 220, ldx_pad=2, ldy_pad=3, ldw_pad=5, w0=True, db=True)], forms=F('dw2')),
        # dW / db starting non-zero
        case('dw', [D(140, 20, 56, w0=True, db=True)], forms=F('dw2')), case('dw', [D(65536, 32, 128, w0=True, db=True)], forms=F('dw4')),
        case('dw', [D(15, 100, 700, w0=True, db=True)], forms=F('dw')),
        # a concatenated X (MG_EINVAL without the MFMA forms)
        case('dw', [D(420, 20, 120, cat=(20, 100), db=True)], forms=F('dw2'), einval_in=('valu', )),
        case('dw', [D(65536, 20, 120, cat=(20, 100), ldx_pad=4)], forms=F('dw4'), einval_in=('valu', )),
        case('dw', [D(140, 100, 64, cat=(8, 12), w0=True)], forms=F('dw'), einval_in=('valu', )),
        # several groups of different classes in one call: runs of one class each
        case('dw', [D(140, 20, 56), D(420, 32, 220, db=True), D(140, 40, 56), D(64, 128, 64, db=True), D(15, 129, 31), D(140, 256, 64, w0=True),
                    D(140, 1, 2, db=True)], forms=F('dw2', 'dw', 'valu_dw')),
        case('dw', [D(65536, 20, 220), D(140, 32, 8, db=True), D(0, 20, 56)], forms=F('dw4')),
        case('dw', [D(17 + i, 20, 56, db=bool(i & 1)) for i in range(70)], forms=F('dw2')),   # more than DW_MAXG = 64 groups of one class
    ]
    return b


# the forms the whole sweep must reach, per profile: one line each, with a shape of the sweep that reaches it.  A threshold that
# moves and orphans a kernel changes the OR of the sweep's masks and fails tests/test_gpu_gemm.py::test_every_reachable_form_ran.
REACHABLE = {
    'default': {
        'rows_unaligned': 'rows 140, N 20, R 25',
        'rows_w4': 'rows 140, N 20, R 56',
        'rows_w16': 'rows 140, N 20, R 220',
        'rows64_rt2': 'rows 16384, N 20, R 56 (two tiles per wave from 16384 rows, i.e. always)',
        'rows_ws': 'rows 16400, N 20, R 220',
        'cols_ws': 'rows 140, N 222, R 20, plain',
        'mfma_cols_exact': 'rows 140, N 220, R 8; R 20 with a bias',
        'mfma_cols_generic': 'rows 140, N 220, R 12',
        'rows_lds': 'rows 8192, N 160, R 128',
        'valu_rows': 'rows 140, N 20, R 4; rows 140, N 129, R 72',
        'dw4': 'rows 65536, N 20, K 220',
        'dw2': 'rows 140, N 20, K 56',
        'dw': 'rows 140, N 20, K 31; N 49 .. 128',
        'valu_dw': 'rows 140, N 129, K 56',
    },
    'valu': {
        'rows_lds': 'rows 16384, N 20, R 56; rows 40000, N 220, R 20',
        'valu_rows': 'rows 140, N 20, R 56; rows 140, N 220, R 20',
        'valu_dw': 'rows 140, N 20, K 56',
    },
    'alt': {
        'rows_unaligned': 'rows 140, N 20, R 25',
        'rows_w4': 'rows 140, N 20, R 56',
        'rows_w16': 'rows 140, N 20, R 220',
        'rows64_rt2': 'rows 16384, N 20, R 56',
        'rows_ws': 'rows 16400, N 20, R 220',
        'cols_ws': 'rows 40000, N 222, R 20: 2500 row tiles on 64 workgroups',
        'mfma_cols_exact': 'rows 140, N 220, R 8',
        'mfma_cols_generic': 'rows 140, N 220, R 12',
        'rows_lds': 'rows 8192, N 160, R 128',
        'valu_rows': 'rows 140, N 20, R 4',
        'dw4': 'rows 140, N 20, K 220 (any row count with MG_DW4_MINROWS=1)',
        'dw2': 'rows 140, N 20, K 56',
        'dw': 'rows 140, N 20, K 31',
        'valu_dw': 'rows 140, N 129, K 56',
    },
}
