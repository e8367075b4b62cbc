"""The join of the deferred weight-gradient flush (csrc/gemm_dispatch.inc: flush_dw, dw_join_wide), planner only, without a GPU.

flush_dw issues the parked weight-gradient groups bucketed by class (N <= 32, <= 48, <= 128, the VALU tiles).  With MG_DW_JOIN_WIDE
(default 1) groups of 33..128 columns leave their bucket and run in the launch of the N <= 32 bucket as 32-column n blocks of
k_gemm_mfma_dw2<2>, under the conditions listed at dw_join_wide.  mg_test_gemm_dw_flush_plan walks that code with the launches
counted instead of issued; mg_test_gemm_dw_plan is the direct path (runs of one class in list order), which never joins and gives
the parent's launches of a bucket when handed that bucket's sub-list.  tests/test_gpu_gemm_dw_join.py runs the same list on the GPU.
"""
import ctypes as C

from tests import gemm_ref as gr
from tests.gemm_ref import D

NARROW = [D(140, 20, 56), D(17, 20, 34), D(420, 32, 220, db=True), D(420, 20, 120, cat=(20, 100), db=True)]
WIDE = [D(140, 128, 128, db=True), D(64, 100, 48), D(300, 65, 144, w0=True, db=True), D(15, 49, 32)]   # eligible
STAY = [D(140, 128, 31), D(140, 128, 64, x_off=1)]   # odd K; X misaligned by 4 bytes
MIXED = NARROW + WIDE + STAY
OFF = b'MG_DW_JOIN_WIDE=0'
BOUND = 2048   # kDwJoinMaxWgs: a wider bucket joins while it plans fewer workgroups than this on its own


def dw_class(n):
    """csrc/gemm_dispatch.inc::dw_class under the default switches"""
    if n <= 128:
        return 1 if n <= 32 else 3 if n <= 48 else 2
    return gr.pick_nt(n)


def _call(fn, groups, switches):
    from molgym_amd import _lib
    arr = gr.dw_groups(gr.build_dw(gr.Case('dw', list(groups)), fill=False))[0]
    mask, n = C.c_uint64(0), C.c_int32(0)
    rc = fn(arr, len(groups), switches, C.byref(mask), C.byref(n))
    assert rc == 0, rc
    return n.value, _lib.gemm_form_names(mask.value)


def flush_plan(lib, groups, switches=b''):
    return _call(lib.mg_test_gemm_dw_flush_plan, groups, switches)


def parent_plan(lib, groups):
    """what the flush launches without the join: every class's sub-list planned on its own by the direct path"""
    total, forms = 0, set()
    for cls in sorted({dw_class(d.N) for d in groups}):
        n, names = _call(lib.mg_test_gemm_dw_plan, [d for d in groups if dw_class(d.N) == cls], OFF)
        total, forms = total + n, forms | names
    return total, forms


def test_mixed_list_joins(built_lib):
    assert flush_plan(built_lib, MIXED) == (2, {'dw2', 'dw'})   # the joined launch + the dword form for the two that stay behind
    assert flush_plan(built_lib, NARROW + WIDE) == (1, {'dw2', 'dw'})   # nothing stays behind: one launch, both form bits
    assert flush_plan(built_lib, NARROW + WIDE + STAY[:1]) == (2, {'dw2', 'dw'})
    assert flush_plan(built_lib, NARROW + WIDE + STAY[1:]) == (2, {'dw2', 'dw'})


def test_switch_off_gives_the_parent_launches(built_lib):
    for groups in (MIXED, NARROW + WIDE, WIDE + NARROW, NARROW, WIDE):
        assert flush_plan(built_lib, groups, OFF) == parent_plan(built_lib, groups)
    assert flush_plan(built_lib, NARROW + WIDE, OFF) == (2, {'dw2', 'dw'})
    assert flush_plan(built_lib, NARROW, OFF) == flush_plan(built_lib, NARROW) == (1, {'dw2'})


def test_no_join_cases(built_lib):
    # the class-1 side with a 65536-row group: the list as it stands still plans the 8-byte form (K = 34 is no multiple of 4), but its
    # row partition would move with the joiners counted, so nothing joins; without the K = 34 group the side plans dw4
    big = NARROW + [D(65536, 20, 220)]
    assert flush_plan(built_lib, big + WIDE + STAY) == parent_plan(built_lib, big + WIDE + STAY) == (2, {'dw2', 'dw'})
    assert flush_plan(built_lib, big + WIDE) == (2, {'dw2', 'dw'})
    big4 = [d for d in big if d.K % 4 == 0]
    assert parent_plan(built_lib, big4) == (1, {'dw4'})
    assert flush_plan(built_lib, big4 + WIDE + STAY) == parent_plan(built_lib, big4 + WIDE + STAY) == (2, {'dw4', 'dw'})
    assert flush_plan(built_lib, big4 + WIDE) == (2, {'dw4', 'dw'})
    # no class-1 group
    assert flush_plan(built_lib, WIDE + STAY) == parent_plan(built_lib, WIDE + STAY) == (1, {'dw'})
    assert flush_plan(built_lib, WIDE) == (1, {'dw'})
    # the wide bucket alone plans at least the bound's workgroups: three 30000 x 128 x 128 groups are 64 rows per wave, ceil(30000 /
    # 256) = 118 row chunks x 8 k tiles = 944 workgroups each (the class-1 side keeps its 64 rows per wave either way: only the
    # bound stands against this join)
    huge = NARROW + WIDE + [D(30000, 128, 128)] * 3
    assert flush_plan(built_lib, huge + STAY) == parent_plan(built_lib, huge + STAY) == (2, {'dw2', 'dw'})
    assert flush_plan(built_lib, huge) == (2, {'dw2', 'dw'})
    assert flush_plan(built_lib, NARROW + WIDE + [D(30000, 128, 128)]) == (1, {'dw2', 'dw'})   # 944 + the small ones: under it
    # one 40000 x 128 x 128 group stays under the bound, but it would move the row partition of the class-1 groups (the launch then
    # plans for 40000 rows): no join either
    moved = NARROW + WIDE + [D(40000, 128, 128)]
    assert flush_plan(built_lib, moved + STAY) == parent_plan(built_lib, moved + STAY) == (2, {'dw2', 'dw'})
    assert flush_plan(built_lib, moved) == (2, {'dw2', 'dw'})


def test_the_bound_is_the_wide_buckets_own_workgroup_count(built_lib):
    """a bucket of 510 x 128 x 128 groups plans 16 rows per wave on its own: ceil(510 / 64) = 8 row chunks x 8 k tiles of 16 = 64
    workgroups a group; 31 of them plan 1984 < 2048 and join, 32 plan exactly 2048 and do not (the class-1 side and its row
    partition are the same in both)"""
    per = 8 * 8
    fewer, more = (BOUND - 1) // per, (BOUND + per - 1) // per
    assert (fewer, more) == (31, 32)
    assert flush_plan(built_lib, NARROW + [D(510, 128, 128)] * fewer) == (1, {'dw2', 'dw'})
    assert flush_plan(built_lib, NARROW + [D(510, 128, 128)] * more) == (2, {'dw2', 'dw'})


def test_class_3_joins_too_and_valu_classes_never(built_lib):
    assert flush_plan(built_lib, NARROW + [D(140, 40, 56)]) == (1, {'dw2', 'dw'})
    assert flush_plan(built_lib, NARROW + [D(140, 40, 56)], OFF) == (2, {'dw2'})   # (<= 48 columns take the 8-byte form on their own)
    assert flush_plan(built_lib, NARROW + [D(140, 129, 56)]) == (2, {'dw2', 'valu_dw'})
    assert flush_plan(built_lib, NARROW[:3] + WIDE, b'MG_MFMA_DW=0')[1] == {'valu_dw'}   # (a concatenated X needs the MFMA forms)


def test_direct_path_did_not_move(built_lib):
    """mg_test_gemm_dw_plan: runs of one class in list order, with and without the switch"""
    runs = 1 + sum(dw_class(a.N) != dw_class(b.N) for a, b in zip(MIXED, MIXED[1:]))
    for sw in (b'', OFF):
        assert _call(built_lib.mg_test_gemm_dw_plan, MIXED, sw) == (runs, {'dw2', 'dw'})
    shuffled = MIXED[::2] + MIXED[1::2]
    runs = 1 + sum(dw_class(a.N) != dw_class(b.N) for a, b in zip(shuffled, shuffled[1:]))
    assert runs > 2
    for sw in (b'', OFF):
        assert _call(built_lib.mg_test_gemm_dw_plan, shuffled, sw)[0] == runs
