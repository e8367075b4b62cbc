"""Superpose structures on the device: the RMSD of two sets of canvases after the best translation and proper rotation.

Relaxation (molgym_amd/relax.py) tells how much energy a sampled molecule drops; how far it moved is this module.  An L-BFGS run is
free to drift and turn a molecule slightly, so the measure is the RMSD after a rigid superposition (Horn's quaternion method),
next to the raw one.  `superpose` / `superpose_canvases` run `mg_superpose` (include/molgym_hip.h; one workgroup of 256 threads per
pair of canvases, one thread per atom, all float64), `superpose_host` is the float64 mirror the kernel is held to bit for bit, and
`relax(..., superpose=True)` / `relax_canvases(..., superpose=True)` issue it behind `mg_pair_relax` on (input, relaxed).

The operation order IS the interface (+ - * /, comparisons, selects and sqrt only -- `1.0 / sqrt(x)`, no reciprocal square root --
float64, contraction off).  R is the workgroup reduction of molgym_amd/relax.py: 256 slots, then v[i] = v[i] + v[i+s] for
s = 128, 64, ..., 1 (Rmax: the larger of the two, a NaN wins).  The selected atoms of a row fill the slots 0 .. m-1 in atom
order -- slot k holds the value of the k-th selected atom; without a mask slot i holds atom i's -- and every other slot holds
+0.0, so a selected subset gives the bits of the subset alone.  Per row with n atoms a_i, b_i, of which m are selected:
  m = R(selected ? 1.0 : 0.0)
  m == 0:  rmsd = displacement = max_deviation = 0.0, the rotation is the identity, the centroids are 0.0, the status is OK and
           `aligned` gets the bytes of B
  centroids     ca_k = R(a_k) / m, cb_k = R(b_k) / m over the selected atoms;  a' = a - ca, b' = b - cb for every atom of the row
  displacement  d = a - b;  D = R((dx*dx + dy*dy) + dz*dz);  displacement = sqrt(D / m)
  covariance    M_kl = R(b'_k * a'_l), nine sums
  Horn's matrix K00 = (Mxx+Myy)+Mzz  K11 = (Mxx-Myy)-Mzz  K22 = (Myy-Mxx)-Mzz  K33 = (Mzz-Mxx)-Myy
                K01 = Myz-Mzy  K02 = Mzx-Mxz  K03 = Mxy-Myx  K12 = Mxy+Myx  K13 = Mzx+Mxz  K23 = Myz+Mzy,  K symmetric
  cyclic Jacobi a full 4 x 4 working copy A = K and V = I; exactly 8 sweeps over (p,q) = (0,1),(0,2),(0,3),(1,2),(1,3),(2,3).  A
                pair whose A_pq == 0.0 is skipped; otherwise
                  th = (A_qq - A_pp) / (2.0*A_pq);  t = 1.0 / (|th| + sqrt(th*th + 1.0)), negated when th < 0
                  c = 1.0 / sqrt(t*t + 1.0);  s = t*c
                  for k = 0..3 the columns  (A_kp, A_kq) <- (c*A_kp - s*A_kq, s*A_kp + c*A_kq)
                  then for k = 0..3 the rows (A_pk, A_qk) <- (c*A_pk - s*A_qk, s*A_pk + c*A_qk)
                  then for k = 0..3 the columns of V as those of A
                (an overflowing th gives t = 0, a rotation that does nothing: intended)
  quaternion    j = the first index of the largest A_jj;  v = V[:, j];  q = v / sqrt(((v0*v0 + v1*v1) + v2*v2) + v3*v3), every
                component negated when q0 < 0;  (w, x, y, z) = q
  rotation      R00 = ((w*w + x*x) - y*y) - z*z   R01 = 2.0*(x*y - w*z)             R02 = 2.0*(x*z + w*y)
                R10 = 2.0*(x*y + w*z)             R11 = ((w*w - x*x) + y*y) - z*z   R12 = 2.0*(y*z - w*x)
                R20 = 2.0*(x*z - w*y)             R21 = 2.0*(y*z + w*x)             R22 = ((w*w - x*x) - y*y) + z*z
  residuals     rb_k = (R_k0*b'_x + R_k1*b'_y) + R_k2*b'_z;  aligned_k = rb_k + ca_k for every atom of the row, selected or not
                res = a' - rb;  r2 = (rx*rx + ry*ry) + rz*rz
                rmsd = sqrt(R(selected ? r2 : 0.0) / m);  max_deviation = sqrt(Rmax(selected ? r2 : 0.0))
The rmsd is taken from the residuals and not from Ga + Gb - 2 lambda, which cancels when the structures nearly coincide.

NONFINITE (m > 0): D is not finite, or one of the 16 entries of A or of the 16 entries of V is not finite after the eighth sweep.
That test covers every sum in front of it: a non-finite A or V entry stays non-finite under a rotation (c >= 1/sqrt(2) is never 0,
so c*inf is inf, and inf - x, a NaN and 0*inf are not finite; a NaN c or s reaches every entry of the two columns of V), every
M_kl is a term of an entry of K, so a non-finite M_kl makes K = A non-finite from the start, and a non-finite centroid component
makes a'_l or b'_k non-finite for every selected atom, and with it a product of every sum M_kl it enters.  Such a row gets NaN in
the three scalars, the rotation and the centroids, and `aligned` gets the bytes of B.  A row whose atom count lies outside 0 .. N
is NONFINITE in the same way, and nothing of it is indexed.  Slots beyond a row's atoms of `aligned` always get the bytes of B.
A NaN or an infinity in an unselected atom takes no part in any sum: the row is OK and that atom's `aligned` is what the
arithmetic gives."""
import ctypes as C
from dataclasses import dataclass
from typing import List

import numpy as np

from . import _lib
from .relax import _tree

OK, NONFINITE = _lib.SUPERPOSE_OK, _lib.SUPERPOSE_NONFINITE
STATUS_NAMES = ('OK', 'NONFINITE')
SWEEPS = 8
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


@dataclass(eq=False)
class Superposed:
    """one superposition of B on A: the RMSD after it, the RMSD before it (`displacement`), the largest distance of a selected
    atom from its partner after it, the proper rotation (3, 3) and the two centroids (3,) with aligned = rotation @ (b - centroid_b)
    + centroid_a, `aligned` (n, 3) float64 for every atom, the status (`STATUS_NAMES`), and `ok`: status == OK"""
    rmsd: float
    displacement: float
    max_deviation: float
    rotation: np.ndarray
    centroid_a: np.ndarray
    centroid_b: np.ndarray
    aligned: np.ndarray
    status: int

    @property
    def ok(self) -> bool:
        return self.status == OK


# ---- the host mirror ---------------------------------------------------------------------------------------------------------------
def _select_mask(select, n: int) -> np.ndarray:
    """`select`: None (every atom), a boolean mask of length n, or a list of atom indices -> a boolean mask"""
    if select is None:
        return np.ones(n, dtype=bool)
    s = np.asarray(select)
    if s.dtype == bool:
        if s.shape != (n, ):
            raise ValueError(f'a select mask of shape {s.shape} for {n} atoms')
        return s.copy()
    mask = np.zeros(n, dtype=bool)
    for k in s.reshape(-1):
        if not 0 <= int(k) < n or int(k) != k:
            raise ValueError(f'selected atom {k} outside 0..{n - 1}')
        mask[int(k)] = True
    return mask


def _pair(a, b):
    a, b = np.array(a, dtype=np.float64), np.array(b, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 3 or b.ndim != 2 or b.shape[1] != 3:
        if not (a.size == 0 and b.size == 0):
            raise ValueError(f'positions of shapes {a.shape} and {b.shape}: two (n, 3) arrays')
        a, b = a.reshape(0, 3), b.reshape(0, 3)
    if len(a) != len(b):
        raise ValueError(f'{len(a)} and {len(b)} atoms: a superposition pairs the atoms slot by slot')
    if len(a) > _lib.MG_MAX_CANVAS:
        raise ValueError(f'a structure of {len(a)} atoms: at most {_lib.MG_MAX_CANVAS}')
    return a, b


def _jacobi(K: np.ndarray):
    """the eight sweeps of the module docstring on a copy of K -> (A, V)"""
    A, V = K.copy(), np.eye(4, dtype=np.float64)
    one, two = np.float64(1.0), np.float64(2.0)
    for _ in range(SWEEPS):
        for p, q in PAIRS:
            apq = A[p, q]
            if apq == 0.0:
                continue
            th = (A[q, q] - A[p, p]) / (two * apq)
            t = one / (np.abs(th) + np.sqrt(th * th + one))
            if th < 0.0:
                t = -t
            c = one / np.sqrt(t * t + one)
            s = t * c
            for k in range(4):
                x, y = A[k, p], A[k, q]
                A[k, p], A[k, q] = c * x - s * y, s * x + c * y
            for k in range(4):
                x, y = A[p, k], A[q, k]
                A[p, k], A[q, k] = c * x - s * y, s * x + c * y
            for k in range(4):
                x, y = V[k, p], V[k, q]
                V[k, p], V[k, q] = c * x - s * y, s * x + c * y
    return A, V


def _rotation(q: np.ndarray) -> np.ndarray:
    w, x, y, z = q
    two = np.float64(2.0)
    return np.array([[((w * w + x * x) - y * y) - z * z, two * (x * y - w * z), two * (x * z + w * y)],
                     [two * (x * y + w * z), ((w * w - x * x) + y * y) - z * z, two * (y * z - w * x)],
                     [two * (x * z - w * y), two * (y * z + w * x), ((w * w - x * x) - y * y) + z * z]], dtype=np.float64)


def _nonfinite(b: np.ndarray) -> 'Superposed':
    nan = float('nan')
    return Superposed(nan, nan, nan, np.full((3, 3), np.nan), np.full(3, np.nan), np.full(3, np.nan), b.copy(), NONFINITE)


def superpose_host(a, b, select=None) -> Superposed:
    """the float64 mirror of `mg_superpose` for one pair of structures (module docstring): B is laid on A.  `select`: a boolean
    mask or atom indices -- the atoms the fit and the three measures are taken over (None: every atom); all atoms are transformed."""
    a, b = _pair(a, b)
    n = len(a)
    sel = _select_mask(select, n)
    with np.errstate(all='ignore'):
        pick = np.flatnonzero(sel)  # the k-th selected atom sits in slot k of every sum
        m = _tree(np.ones(len(pick)))
        if m == 0.0:
            return Superposed(0.0, 0.0, 0.0, np.eye(3), np.zeros(3), np.zeros(3), b.copy(), OK)
        ca = np.array([_tree(a[pick, k]) / m for k in range(3)])
        cb = np.array([_tree(b[pick, k]) / m for k in range(3)])
        a1, b1, d = a - ca, b - cb, (a - b)[pick]
        D = _tree((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        M = np.array([[_tree(b1[pick, k] * a1[pick, l]) for l in range(3)] for k in range(3)])
        (xx, xy, xz), (yx, yy, yz), (zx, zy, zz) = M
        K = np.zeros((4, 4), dtype=np.float64)
        K[0, 0], K[1, 1], K[2, 2], K[3, 3] = (xx + yy) + zz, (xx - yy) - zz, (yy - xx) - zz, (zz - xx) - yy
        K[0, 1] = K[1, 0] = yz - zy
        K[0, 2] = K[2, 0] = zx - xz
        K[0, 3] = K[3, 0] = xy - yx
        K[1, 2] = K[2, 1] = xy + yx
        K[1, 3] = K[3, 1] = zx + xz
        K[2, 3] = K[3, 2] = yz + zy
        A, V = _jacobi(K)
        if not (np.isfinite(D) and np.isfinite(A).all() and np.isfinite(V).all()):
            return _nonfinite(b)
        j = 0
        for k in range(1, 4):
            if A[k, k] > A[j, j]:
                j = k
        v = V[:, j]
        q = v / np.sqrt(((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + v[3] * v[3])
        if q[0] < 0.0:
            q = -q
        rot = _rotation(q)
        rb = np.stack([(rot[k, 0] * b1[:, 0] + rot[k, 1] * b1[:, 1]) + rot[k, 2] * b1[:, 2] for k in range(3)], axis=1).reshape(n, 3)
        aligned = rb + ca
        res = a1 - rb
        res = res[pick]
        r2 = (res[:, 0] * res[:, 0] + res[:, 1] * res[:, 1]) + res[:, 2] * res[:, 2]
        rmsd = np.sqrt(_tree(r2) / m)
        dev = np.sqrt(_tree(r2, larger=True))
        return Superposed(float(rmsd), float(np.sqrt(D / m)), float(dev), rot, ca, cb, aligned, OK)


# ---- the device ----------------------------------------------------------------------------------------------------------------------
def _device_call(pos_a, pos_b, natoms_dev, select, out):
    """checks of the device entry point's tensors -> (E, N, select as uint8 or None)"""
    import torch
    for name, t in (('pos_a', pos_a), ('pos_b', pos_b)):
        if t.dtype != torch.float64 or t.dim() != 3 or t.shape[2] != 3 or not t.is_contiguous():
            raise ValueError(f'{name}: a contiguous [E][N][3] float64 tensor')
    if pos_b.shape != pos_a.shape:
        raise ValueError(f'pos_a {tuple(pos_a.shape)} and pos_b {tuple(pos_b.shape)}: the same shape')
    E, N = int(pos_a.shape[0]), int(pos_a.shape[1])
    if not 1 <= N <= _lib.MG_MAX_CANVAS or E < 1:
        raise ValueError(f'{E} canvases of {N} slots: at least one canvas, 1..{_lib.MG_MAX_CANVAS} slots')
    if natoms_dev.dtype != torch.int32 or tuple(natoms_dev.shape) != (E, ) or not natoms_dev.is_contiguous():
        raise ValueError(f'natoms_dev: a contiguous [{E}] int32 tensor')
    if select is not None:
        if select.dtype not in (torch.bool, torch.uint8) or tuple(select.shape) != (E, N) or not select.is_contiguous():
            raise ValueError(f'select: a contiguous [{E}][{N}] bool tensor')
        select = select.view(torch.uint8)
    if out is not None:
        if out.dtype != torch.float64 or out.shape != pos_a.shape or not out.is_contiguous():
            raise ValueError('out: a contiguous float64 tensor of the shape of pos_a')
        if out.data_ptr() == pos_a.data_ptr():
            raise ValueError('out may be pos_b, not pos_a')
    for t in (pos_b, natoms_dev) + tuple(x for x in (select, out) if x is not None):
        if t.device != pos_a.device:
            raise ValueError('the tensors lie on different devices')
    return E, N, select


def _superpose_launch(pos_a, pos_b, natoms_dev, select, aligned, scalars, frame, status):
    """one `mg_superpose` on the current stream of the tensors' device; `scalars`: the three [E] outputs, `frame`: the rotation
    [E][9] and the two centroids [E][3]"""
    import torch
    E, N = int(pos_a.shape[0]), int(pos_a.shape[1])
    dev = pos_a.device
    p = _lib.ptr
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().mg_superpose(E, N, p(pos_a), p(pos_b), p(natoms_dev), None if select is None else p(select),
                                           None if aligned is None else p(aligned), *[p(s) for s in scalars], *[p(f) for f in frame],
                                           p(status), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))


def superpose_canvases(pos_a, pos_b, natoms_dev, select=None, out=None) -> dict:
    """`mg_superpose` on device tensors (pos_a, pos_b [E][N][3] float64, natoms_dev [E] int32, select [E][N] bool or None), for
    example a `DeviceEpisodes.canvas` and its relaxed positions; nothing is copied to the host.  `out`: the [E][N][3] float64
    tensor B laid on A goes to (it may be `pos_b` itself, not `pos_a`; None: a new one).  Device tensors `aligned`, `rmsd`,
    `displacement`, `max_deviation` (float64 [E]), `rotation` [E][3][3], `centroid_a`, `centroid_b` [E][3], `status` (int32 [E])."""
    import torch
    E, N, select = _device_call(pos_a, pos_b, natoms_dev, select, out)
    dev = pos_a.device
    if out is None:
        out = torch.empty_like(pos_a)
    f = torch.empty((3, E), dtype=torch.float64, device=dev)
    rot = torch.empty((E, 3, 3), dtype=torch.float64, device=dev)
    cen = torch.empty((2, E, 3), dtype=torch.float64, device=dev)
    status = torch.empty(E, dtype=torch.int32, device=dev)
    _superpose_launch(pos_a, pos_b, natoms_dev, select, out, (f[0], f[1], f[2]), (rot, cen[0], cen[1]), status)
    return dict(aligned=out, rmsd=f[0], displacement=f[1], max_deviation=f[2], rotation=rot, centroid_a=cen[0], centroid_b=cen[1],
                status=status)


def _positions(s) -> np.ndarray:
    """an (n, 3) array, an `Episode` or a `Relaxed` -> its positions"""
    return s.positions if hasattr(s, 'positions') else s


def superpose(A, B, select=None, device=None) -> List[Superposed]:
    """Lay every structure of `B` on its partner in `A` -- lists of (n, 3) arrays, `Episode`s or `Relaxed` -- on the device: packed
    into canvases sized to the largest of them, one upload, one `mg_superpose`, one copy back.  `select`: one mask or index list for
    all pairs, or one per pair.  ValueError: lists of unequal length, partners of unequal atom counts, more than 255 atoms, a
    `select` out of range."""
    A, B = list(A), list(B)
    if len(A) != len(B):
        raise ValueError(f'{len(A)} structures to lay {len(B)} on')
    pairs = [_pair(_positions(a), _positions(b)) for a, b in zip(A, B)]
    E = len(pairs)
    if E == 0:
        return []
    per_pair = select is not None and len(select) > 0 and not np.isscalar(select[0])
    if per_pair and len(select) != E:
        raise ValueError(f'{len(select)} selections for {E} pairs')
    masks = [_select_mask(select[k] if per_pair else select, len(a)) for k, (a, _) in enumerate(pairs)]
    import torch
    N = max(1, max(len(a) for a, _ in pairs))
    # ONE upload: [positions A f64 | positions B f64 | atom counts i32 | select u8], every section 8-byte aligned
    o_b = E * N * 24
    o_n = 2 * o_b
    o_s = o_n + (E * 4 + 7) // 8 * 8
    host = np.zeros(o_s + E * N, dtype=np.uint8)
    pa, pb = host[:o_b].view(np.float64).reshape(E, N, 3), host[o_b:o_n].view(np.float64).reshape(E, N, 3)
    nat, sl = host[o_n:o_n + E * 4].view(np.int32), host[o_s:].reshape(E, N)
    for k, (a, b) in enumerate(pairs):
        n = len(a)
        pa[k, :n], pb[k, :n], nat[k], sl[k, :n] = a, b, n, masks[k]
    dev = torch.device('cuda' if device is None else device)
    if dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    block = torch.from_numpy(host).to(dev)
    d_a, d_b = block[:o_b].view(torch.float64).view(E, N, 3), block[o_b:o_n].view(torch.float64).view(E, N, 3)
    d_nat, d_sel = block[o_n:o_n + E * 4].view(torch.int32), block[o_s:].view(E, N)
    # ONE copy back: [aligned | rmsd | displacement | max deviation | rotation | centroid A | centroid B | status]
    o_f = E * N * 24
    o_i = o_f + 18 * E * 8
    back = torch.empty(o_i + E * 4, dtype=torch.uint8, device=dev)
    f = back[o_f:o_i].view(torch.float64)
    _superpose_launch(d_a, d_b, d_nat, d_sel, back[:o_f].view(torch.float64).view(E, N, 3), (f[:E], f[E:2 * E], f[2 * E:3 * E]),
                      (f[3 * E:12 * E], f[12 * E:15 * E], f[15 * E:18 * E]), back[o_i:].view(torch.int32))
    got = back.cpu().numpy()
    h_al, h_f, h_i = got[:o_f].view(np.float64).reshape(E, N, 3), got[o_f:o_i].view(np.float64), got[o_i:].view(np.int32)
    return [Superposed(float(h_f[k]), float(h_f[E + k]), float(h_f[2 * E + k]), h_f[3 * E + 9 * k:3 * E + 9 * k + 9].reshape(3, 3).copy(),
                       h_f[12 * E + 3 * k:12 * E + 3 * k + 3].copy(), h_f[15 * E + 3 * k:15 * E + 3 * k + 3].copy(),
                       h_al[k, :len(a)].copy(), int(h_i[k])) for k, (a, _) in enumerate(pairs)]
