"""The Python layer that drives the library, on the host alone: what the two agents share (molgym_amd/agents/base.py), the one
`IntCfg` constructor, the section packer and the host mirror of a committed canvas step.  Agents are made with `__new__`, as in
tests/test_host.py: no device, no parameters."""
import numpy as np
import pytest

from molgym_amd import _lib
from molgym_amd.agents.base import check_action_rows
from molgym_amd.agents.canvas import DeviceCanvas
from molgym_amd.agents.covariant import CovariantAC
from molgym_amd.agents.internal import SchNetAC, gather_totals


def _bare_schnet(canvas_size, zs=(0, 1, 6)):
    ac = SchNetAC.__new__(SchNetAC)
    ac.zs, ac.num_zs, ac.num_atoms, ac.network_width = list(zs), len(zs), canvas_size, 32
    ac.min_distance, ac.max_distance = 0.9, 1.8
    return ac


# ---- SchNetAC._cfg --------------------------------------------------------------------------------------------------------------
def test_cfg_totals_are_gather_totals_and_the_offsets_of_assemble():
    ac, natoms = _bare_schnet(5), np.array([0, 1, 2, 5])
    cfg = ac._cfg(natoms)
    assert (cfg.TA, cfg.MA, cfg.ME) == gather_totals(natoms) == (8, 32, 98)
    sizes = np.concatenate([natoms, natoms + 1, natoms + 1]).astype(np.int64)  # (as `_assemble` lays the 3B molecules out)
    mol_off, edge_off = np.concatenate([[0], np.cumsum(sizes)]), np.concatenate([[0], np.cumsum(sizes * (sizes - 1))])
    assert mol_off.dtype == edge_off.dtype == np.int64 and cfg.MA == mol_off[-1] and cfg.ME == edge_off[-1]
    assert (cfg.B, cfg.N, cfg.Z, cfg.W) == (4, 5, 3, 32) and list(cfg.zs)[:3] == [0, 1, 6]
    assert cfg.min_distance == np.float32(0.9) and cfg.max_distance == np.float32(1.8)
    alias = ac._canvas_cfg(natoms)
    assert bytes(alias) == bytes(cfg)


def test_cfg_refuses_two_to_the_31_pairs_on_every_route():
    ac = _bare_schnet(255)
    assert 11000 * (3 * 255 * 255 + 255) == 2_148_630_000 >= 2**31
    for route in (ac._cfg, ac._canvas_cfg):
        with pytest.raises(ValueError, match='2\\^31'):
            route(np.full(11000, 255))
        assert route(np.full(10990, 255)).ME == 10990 * 195330 < 2**31


# ---- check_action_rows ----------------------------------------------------------------------------------------------------------
LAYOUTS = [(6, 0, 1), (7, 1, 2)]  # (columns, focus column, element column) of CovariantAC's and SchNetAC's rows


@pytest.mark.parametrize('cols,fc,ec', LAYOUTS)
def test_action_rows_check(cols, fc, ec):
    N, Z = 5, 3
    empty = check_action_rows(np.zeros((0, cols)), 0, cols, fc, ec, N, Z)
    assert empty.shape == (0, cols) and empty.dtype == np.float32
    rows = np.zeros((3, cols), dtype=np.float64)
    rows[:, fc], rows[:, ec] = [0, N - 1, 2], [Z - 1, 0, 1]
    got = check_action_rows(rows, 3, cols, fc, ec, N, Z)
    assert got.dtype == np.float32 and got.flags['C_CONTIGUOUS'] and np.array_equal(got, rows.astype(np.float32))
    for col, bad in ((fc, -1), (fc, N), (ec, -1), (ec, Z)):
        wrong = rows.copy()
        wrong[1, col] = bad
        with pytest.raises(RuntimeError, match='index out of range in one-hot selection'):
            check_action_rows(wrong, 3, cols, fc, ec, N, Z)
    with pytest.raises(AssertionError):
        check_action_rows(rows, 2, cols, fc, ec, N, Z)
    with pytest.raises(AssertionError):
        check_action_rows(rows[:, :-1], 3, cols, fc, ec, N, Z)


def test_the_agents_check_their_own_layouts():
    cov = CovariantAC.__new__(CovariantAC)
    cov.zs = [0, 1, 6]
    cov.observation_space = type('Space', (), {'canvas_space': type('Canvas', (), {'size': 5})})
    assert cov._check_actions(np.zeros((0, 6)), 0).shape == (0, 6)
    with pytest.raises(RuntimeError, match='one-hot'):
        cov._check_actions(np.array([[5.0, 0, 1, 0, 0, 1]]), 1)
    ia = _bare_schnet(5)
    parsed = (np.zeros((0, 5), np.int32), np.zeros((0, 3), np.float32), np.zeros(0, np.int64), np.zeros((0, 5, 3)))
    assert ia._placements(parsed, np.zeros((0, 7)))[0].shape == (0, 7)  # (an empty batch: no .min() of nothing)


# ---- _lib.sections --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sizes,align', [((0, 1, 63, 64, 65), 256), ((5, 5, 9, 27, 12, 28), 4), ((7, ), 64), ((), 16)])
def test_sections_are_aligned_and_disjoint(sizes, align):
    offs, total = _lib.sections(sizes, align)
    assert len(offs) == len(sizes) and all(o % align == 0 for o in offs) and total % align == 0
    ends = [o + n for o, n in zip(offs, sizes)]
    assert all(e <= nxt for e, nxt in zip(ends, offs[1:] + [total]))


def test_sections_totals_of_the_existing_buffers():
    # FlatThetaAgent._upload_packed: 4-byte words, sections of 64 words = 256 bytes
    offs, total = _lib.sections((0, 1, 63, 64, 65), 64)
    assert offs == [0, 0, 64, 128, 192] and total == 320 and total * 4 == 1280
    # SchNetAC._assemble before it went through _upload_packed, IntRolloutOnDevice.minibatch: words, sections of 4 words = 16 bytes
    offs, total = _lib.sections((5, 5, 9, 27, 12, 28), 4)
    assert offs == [0, 8, 16, 28, 56, 68] and total == 96 and total * 4 == 384


# ---- pickling -------------------------------------------------------------------------------------------------------------------
def _empty(ac):
    return {name: empty and empty() for name, empty in ac._TRANSIENT}


@pytest.mark.parametrize('cls', [CovariantAC, SchNetAC])
def test_transient_attributes_never_reach_a_pickle_and_come_back_empty(cls):
    names = [name for name, _ in cls._TRANSIENT]
    for must in ('_ws_cache', '_ws_epoch', '_last_ws', '_last_cfg', '_last_out', '_last_gout', 'last_step_used_graph'):
        assert must in names
    assert ('_last_sample_cfg' in names and '_draw_par_c' in names) if cls is SchNetAC else \
        ('_unchecked' in names and '_grad_k' in names and '_iota' in names)
    ac = cls.__new__(cls)
    ac.zs, ac.kept = [0, 1, 6], 'kept'
    sentinels = {name: object() for name in names}
    for name, s in sentinels.items():
        setattr(ac, name, s)
    state = ac.__getstate__()
    assert state['kept'] == 'kept' and state['zs'] == [0, 1, 6]
    assert not any(v is s for v in state.values() for s in sentinels.values()) and not set(names) & set(state)
    for name, s in sentinels.items():  # (taking the state left the object as it was)
        assert getattr(ac, name) is s
    # the state just taken; the same with nothing of the caches in it (an old pickle); and what the parent commit wrote
    for saved in (state, {k: v for k, v in state.items() if k not in names}, dict(state, _last_ws=None, _ws_cache={})):
        new = cls.__new__(cls)
        new.__setstate__(dict(saved))
        assert new.kept == 'kept'
        for name, want in _empty(new).items():
            got = new.__dict__[name]
            assert got == want and type(got) is type(want), name
        assert new._ws_cache is not new._ws_epoch
    # a cache that was taken out of the instance is empty again on its next use
    new.__dict__.pop('_ws_epoch')  # (as tests/test_gpu_covariant_ordered_edges.py forgets an epoch)
    assert new._ws_epoch == {} and '_ws_epoch' in new.__dict__
    with pytest.raises(AttributeError):
        new.no_such_attribute


# ---- DeviceCanvas.commit_mirror -------------------------------------------------------------------------------------------------
def test_commit_mirror_follows_the_placed_rows():
    cv = DeviceCanvas.__new__(DeviceCanvas)
    cv.zs, cv.N, cv.E = [0, 1, 6], 3, 4
    cv.natoms = np.array([1, 2, 3, 0], dtype=np.int32)
    cv.bags_host = np.array([[0, 2, 1], [0, 1, 1], [0, 1, 1], [0, 0, 2]], dtype=np.int64)
    cv.last_placed = None
    # row 0 places a hydrogen, row 1 draws the null element, row 2's canvas is full, row 3's is empty and takes a carbon
    elements = np.array([1, 0, 2, 2], dtype=np.int64)
    positions = np.arange(12, dtype=np.float32).reshape(4, 3)
    before = cv.natoms.copy()
    cv.commit_mirror(before, elements, positions)
    assert cv.natoms.dtype == np.int32 and cv.natoms.tolist() == [2, 2, 3, 1] and before.tolist() == [1, 2, 3, 0]
    assert cv.bags_host.tolist() == [[0, 1, 1], [0, 1, 1], [0, 1, 1], [0, 0, 1]]
    placed, where = cv.last_placed
    assert placed.dtype == bool and placed.tolist() == [True, False, False, True]
    assert where.dtype == np.float64 and np.array_equal(where, positions) and not np.shares_memory(where, positions)
