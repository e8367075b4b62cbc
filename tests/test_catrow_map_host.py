"""The stored rows of the atom cat-mix (levels >= 1), no GPU.

A logical row of a channel is [ag: nblk_l | in: 1 | sq: nblk_l]; sq is the channel-wise CG product of the atom's representation
with itself, so block (l2, l1) -> l equals (-1)^(l1 + l2 - l) times block (l1, l2) -> l and a diagonal block with odd l vanishes.
The library stores ag, in and the sq blocks with l1 < l2 or (l1 == l2, l even); mg_test_catrow_map returns the map as the kernels,
the weight preparation and the gradient fold evaluate it.  Here it is compared with a Python enumeration of the blocks, and the
rule itself is pinned to the float64 oracle (oracle.so3.cg_product), not to this code."""
import ctypes as C

import numpy as np
import pytest
import torch

from molgym_amd import _lib
from oracle import so3

MAXL = 4
NBLK = [5, 12, 16, 17, 15]
WIDTHS = [11, 17, 27, 25, 25]


def blocks(l):
    """(l1, l2) blocks of output degree l, l1 outer / l2 inner: the order of oracle.so3.cg_product and of gen_tables.py"""
    return [(l1, l2) for l1 in range(MAXL + 1) for l2 in range(MAXL + 1) if abs(l1 - l2) <= l <= min(l1 + l2, MAXL)]


def expected_map():
    """per degree: (logical column of every stored column, {logical column: (stored column, sign)}; dropped columns: (-1, 0))"""
    out = []
    for l in range(MAXL + 1):
        bl = blocks(l)
        nb = len(bl)
        assert nb == NBLK[l]
        logical = list(range(nb + 1))
        kept = [bp for bp, (l1, l2) in enumerate(bl) if l1 < l2 or (l1 == l2 and l % 2 == 0)]
        logical += [nb + 1 + bp for bp in kept]
        serve = {col: (col, 1) for col in range(nb + 1)}
        for bp, (l1, l2) in enumerate(bl):
            col = nb + 1 + bp
            if bp in kept:
                serve[col] = (nb + 1 + kept.index(bp), 1)
            elif l1 > l2:
                serve[col] = (nb + 1 + kept.index(bl.index((l2, l1))), (-1) ** (l1 + l2 - l))
            else:
                serve[col] = (-1, 0)
        out.append((logical, serve))
    return out


@pytest.fixture(scope='module')
def lib_map(built_lib):
    w = (C.c_int32 * 5)()
    lo = (C.c_int32 * 160)()
    st = (C.c_int32 * 320)()
    sg = (C.c_int32 * 320)()
    _lib.check(built_lib.mg_test_catrow_map(w, lo, st, sg), built_lib)
    return list(w), np.array(lo).reshape(5, 32), np.array(st).reshape(5, 64), np.array(sg).reshape(5, 64)


def test_widths_and_slice(lib_map):
    w = lib_map[0]
    assert w == WIDTHS
    assert sum((2 * l + 1) * w[l] for l in range(5)) == 597
    assert sum((2 * l + 1) * (2 * NBLK[l] + 1) for l in range(5)) == 775
    assert [w[l] - NBLK[l] - 1 for l in range(5)] == [5, 4, 10, 7, 9]


def test_map_matches_block_enumeration(lib_map):
    w, lo, st, sg = lib_map
    for l, (logical, serve) in enumerate(expected_map()):
        assert list(lo[l, :w[l]]) == logical and (lo[l, w[l]:] == -1).all()
        W = 2 * NBLK[l] + 1
        for col in range(W):
            assert (int(st[l, col]), int(sg[l, col])) == serve[col], (l, col)
        assert (st[l, W:] == -1).all() and (sg[l, W:] == 0).all()
        # every stored column is hit exactly once as "kept": by the logical column it holds, with sign +1
        hits = [0] * w[l]
        for cs, col in enumerate(logical):
            assert st[l, col] == cs and sg[l, col] == 1
            hits[cs] += 1
        assert hits == [1] * w[l]
        # every logical sq column is kept, mirrored or dropped; the dropped ones are the odd-l diagonals
        kinds = {'kept': 0, 'mirrored': 0, 'dropped': 0}
        for bp, (l1, l2) in enumerate(blocks(l)):
            col = NBLK[l] + 1 + bp
            if st[l, col] < 0:
                assert l1 == l2 and l % 2 == 1
                kinds['dropped'] += 1
            elif lo[l, st[l, col]] == col:
                kinds['kept'] += 1
            else:
                assert l1 > l2 and abs(sg[l, col]) == 1
                kinds['mirrored'] += 1
        assert kinds['kept'] == w[l] - NBLK[l] - 1 and sum(kinds.values()) == NBLK[l]


def test_rule_holds_in_the_oracle(lib_map):
    """cg_product(rep, rep) of the float64 oracle obeys the rule the map encodes: a mirrored block is s times its partner, a
    dropped block is zero, to 1e-12 of the largest entry"""
    w, lo, st, sg = lib_map
    tau = 3
    g = torch.Generator().manual_seed(5)
    rep = so3.SO3Vec([torch.randn(2, tau, 2 * l + 1, 2, generator=g, dtype=torch.float64) for l in range(MAXL + 1)])
    cg = so3.CGTable(MAXL, dtype=torch.float64)
    sq = so3.cg_product(cg, rep, rep, MAXL)
    scale = max(p.abs().max().item() for p in sq)
    for l in range(MAXL + 1):
        part = sq[l].reshape(2, NBLK[l], tau, 2 * l + 1, 2)  # channel axis: block-major
        for bp in range(NBLK[l]):
            col = NBLK[l] + 1 + bp
            if st[l, col] < 0:
                assert part[:, bp].abs().max().item() <= 1e-12 * scale, (l, bp)
            else:
                src = int(lo[l, st[l, col]]) - NBLK[l] - 1
                assert (part[:, bp] - int(sg[l, col]) * part[:, src]).abs().max().item() <= 1e-12 * scale, (l, bp)


def test_workspace_shrinks(built_lib):
    """a cfg2-shaped call (140 canvases of 7 slots, 510 atoms): the rows of the two upper levels, their adjoint and the expanded
    gradients of their mixes lose 178 of 775 complex per atom and channel"""
    from molgym_amd.synthetic import CONFIGS
    cfg2 = CONFIGS['cfg2']
    hid, per = C.c_int32(), C.c_int32()
    _lib.check(built_lib.mg_cov_channels(C.byref(hid), C.byref(per)), built_lib)
    CH = hid.value
    ld = lambda width: (2 * CH * width + 31) // 32 * 32
    TA = 510
    cfg = _lib.CovCfg()
    cfg.B, cfg.N, cfg.Z = 140, cfg2['canvas_size'], len(cfg2['zs'])
    cfg.TA, cfg.TE = TA, TA * (cfg2['canvas_size'] - 1)
    cfg.W, cfg.G = 128, 3
    for i, z in enumerate(cfg2['zs']):
        cfg.zs[i] = z
    cfg.has_beta, cfg.beta, cfg.bag_scale = 1, -10.0, 5.0
    cfg.min_distance, cfg.max_distance = 0.8, 1.8
    n = C.c_size_t()
    _lib.check(built_lib.mg_cov_workspace_bytes(C.byref(cfg), C.byref(n)), built_lib)
    off, cnt = C.c_int64(), C.c_int64()
    for l in range(5):
        for k in (1, 2):
            _lib.check(built_lib.mg_cov_workspace_lookup(C.byref(cfg), f'cat_a{k}_{l}'.encode(), C.byref(off), C.byref(cnt)), built_lib)
            assert cnt.value == TA * (2 * l + 1) * ld(WIDTHS[l]) + 4
            assert cnt.value <= TA * (2 * l + 1) * ld(2 * NBLK[l] + 1) + 4
    # against the logical layout: three matrices of rows per atom (two levels forward, one adjoint buffer)
    old_rows = sum(TA * (2 * l + 1) * ld(2 * NBLK[l] + 1) for l in range(5))
    new_rows = sum(TA * (2 * l + 1) * ld(WIDTHS[l]) for l in range(5))
    assert new_rows < old_rows
    _lib.check(built_lib.mg_cov_workspace_lookup(C.byref(cfg), b'd_cat_a', C.byref(off), C.byref(cnt)), built_lib)
    assert cnt.value <= new_rows + 5 * 64 + 64
    if CH == 10:
        assert new_rows * 4 == TA * 48768 and old_rows * 4 == TA * 63232
        # the whole workspace of this call with the logical rows (recorded from the library before the change): 163 339 520 bytes;
        # three row matrices per atom shrink, and the expanded gradients and derived weights of ten mixes
        assert n.value <= 163339520 - 3 * (old_rows - new_rows) * 4
