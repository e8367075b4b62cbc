"""mg_int_gather_batch, called through the C ABI: the ragged 3B-molecule batch of the rows `idx` of a parked rollout against
`SchNetAC._assemble` on the same host rows with `placed` taken from `mg_int_place` (existing code) -- every output bit for bit,
every output between guard bands -- and the appended atoms against the host's float64 helper; the handled bad input."""
import ctypes as C

import numpy as np
import pytest
import torch

from molgym_amd import _lib
from molgym_amd.agents.covariant import compact_canvases, observation_arrays
from molgym_amd.agents.internal import gather_totals
from molgym_amd.spaces import ActionSpace, ObservationSpace
from molgym_amd.synthetic import make_batch_internal
from tests.test_gpu_internal_canvas import _place_dev, _place_host, _sf6

pytestmark = pytest.mark.gpu
ZS = [0, 9, 16]
GUARD = 4096
EINVAL = -1
_CACHE = {}


def _ac(canvas):
    if ('ac', canvas) not in _CACHE:
        from molgym_amd.agents.internal import SchNetAC
        torch.manual_seed(0)
        _CACHE['ac', canvas] = SchNetAC(ObservationSpace(canvas, ZS), ActionSpace(ZS), (0.8, 1.8), 64, device='cuda:0')
    return _CACHE['ac', canvas]


def _finish(pos, charges, natoms, bags, acts, seed):
    """the host rows, their placements by mg_int_place and by the host helper (computed once), and the rows parked in HBM"""
    rng = np.random.default_rng(seed)
    S = len(natoms)
    host = dict(pos=pos, charges=charges.astype(np.int32), natoms=natoms.astype(np.int64), bags=bags.astype(np.float32),
                acts=np.ascontiguousarray(acts, dtype=np.float32), logp=rng.normal(-5.0, 1.0, size=S), adv=rng.normal(size=S),
                ret=rng.normal(0.0, 0.3, size=S))
    host['z_new'] = np.asarray(ZS, dtype=np.int32)[np.rint(host['acts'][:, 2]).astype(np.int64)]
    host['dev_plus'], host['dev_minus'] = _place_dev(pos, natoms, host['acts'])
    host['ref_plus'], host['ref_minus'] = _place_host(pos, natoms, host['acts'])
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).cuda()
    park = dict(s_pos64=up(pos, np.float64), s_charges=up(charges, np.int32), s_natoms=up(natoms, np.int32),
                s_bags=up(bags, np.float32), s_actions=up(host['acts'], np.float32), s_logp=up(host['logp'], np.float64),
                s_adv=up(host['adv'], np.float64), s_ret=up(host['ret'], np.float64))
    return host, park


def _rollout9():
    """make_batch_internal(40, 9): n = 0 and n = N by construction; rows 2..7 get 1, 2, 3 atoms; rows 10..16 are the exact SF6
    octahedron with each of its seven atoms as the focus (ties among the nearest atoms everywhere)"""
    if 9 not in _CACHE:
        S, N = 40, 9
        d = make_batch_internal(S, N, ZS, seed=21)
        labels, xyz, bags = observation_arrays(d['obs'], ZS, N)
        pos, charges, natoms = compact_canvases(labels, xyz, ZS)
        acts = np.asarray(d['act'], dtype=np.float32)
        rng = np.random.default_rng(3)
        for r, n in zip(range(2, 8), (1, 2, 3, 1, 2, 3)):
            pos[r, :n] = rng.normal(scale=1.5, size=(n, 3))
            pos[r, n:], charges[r, :n], charges[r, n:], natoms[r] = 0.0, 9, 0, n
            acts[r, 1] = rng.integers(0, n)
        for f in range(7):
            r = 10 + f
            pos[r], charges[r] = 0.0, 0
            pos[r, :7], charges[r, :7], natoms[r] = _sf6([0, 1, 2, 3, 4, 5]), [16] + [9] * 6, 7
            acts[r, 1] = f
        assert natoms[0] == 0 and natoms[1] == N
        _CACHE[9] = _finish(pos, charges, natoms, bags, acts, seed=4)
    return _CACHE[9]


def _rollout255():
    """the boundaries of a 64-lane atom loop"""
    if 255 not in _CACHE:
        N = 255
        natoms = np.array([0, 63, 64, 65, 200, 255])
        S = len(natoms)
        rng = np.random.default_rng(8)
        pos = rng.normal(scale=4.0, size=(S, N, 3))
        charges = rng.choice([9, 16], size=(S, N))
        real = np.arange(N)[None, :] < natoms[:, None]
        pos[~real], charges[~real] = 0.0, 0
        bags = rng.integers(0, 4, size=(S, len(ZS)))
        acts = np.zeros((S, 7), dtype=np.float32)
        acts[:, 1] = [rng.integers(0, max(n, 1)) for n in natoms]
        acts[:, 2] = rng.integers(1, len(ZS), size=S)
        acts[:, 3], acts[:, 4], acts[:, 5] = rng.uniform(0.8, 1.8, S), rng.uniform(0.3, 2.8, S), rng.uniform(-3.0, 3.0, S)
        acts[:, 6] = rng.integers(0, 2, size=S)
        _CACHE[255] = _finish(pos, charges, natoms, bags, acts, seed=9)
    return _CACHE[255]


class _Guarded:
    """an output of exactly `numel` elements, prefilled with 0xFF, between two guard bands of 0xA5"""

    def __init__(self, numel, dtype):
        self.nbytes = numel * torch.empty(0, dtype=dtype).element_size()
        self.big = torch.full((GUARD + self.nbytes + GUARD, ), 0xA5, dtype=torch.uint8, device='cuda')
        self.big[GUARD:GUARD + self.nbytes].fill_(0xFF)
        self.t = self.big[GUARD:GUARD + self.nbytes].view(dtype)

    def intact(self):
        return bool((self.big[:GUARD] == 0xA5).all()) and bool((self.big[GUARD + self.nbytes:] == 0xA5).all())


class _Same:
    """(for the refusals: every output pointer is the same poisoned buffer)"""

    def __init__(self, buf):
        self.t = buf


PARKED = ('s_pos64', 's_charges', 's_natoms', 's_bags', 's_actions', 's_logp', 's_adv', 's_ret')
NAMES = ('mol_off', 'edge_off', 'molZ', 'molpos', 'bags', 'actions', 'logp', 'adv', 'ret')


def _outputs(B, MA, Z):
    i32, f32, f64 = torch.int32, torch.float32, torch.float64
    sizes = dict(mol_off=(3 * B + 1, i32), edge_off=(3 * B + 1, i32), molZ=(MA, i32), molpos=(3 * MA, f32), bags=(B * Z, f32),
                 actions=(7 * B, f32), logp=(B, f64), adv=(B, f64), ret=(B, f64))
    return {k: _Guarded(*sizes[k]) for k in NAMES}


def _call(park, N, B, idx, totals, out, err, S=None, Z=len(ZS), replace=None):
    p = lambda t: C.c_void_p(None if t is None else t.data_ptr())
    src = dict(park, **{k: g.t for k, g in out.items()}, idx=idx, err=err)
    src.update(replace or {})
    zs = (C.c_int32 * _lib.MG_MAX_Z)(*ZS)
    S = park['s_natoms'].numel() if S is None else S
    order = ('idx', ) + PARKED + NAMES + ('err', )
    assert len(src) == len(order)
    return _lib.lib().mg_int_gather_batch(B, N, Z, S, *totals, zs, *(p(src[k]) for k in order),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream))


def _gather(park, N, natoms_host, idx, totals=None):
    """one call on guarded outputs: (outputs, err, the guards)"""
    rows = np.arange(len(natoms_host)) if idx is None else np.asarray(idx)
    B = len(rows)
    if totals is None:
        totals = gather_totals(natoms_host[rows])
    out = _outputs(B, totals[1], len(ZS))
    err = torch.zeros(1, dtype=torch.int32, device='cuda')
    idx_dev = None if idx is None else torch.from_numpy(np.asarray(idx, dtype=np.int64)).cuda()
    _lib.check(_call(park, N, B, idx_dev, totals, out, err))
    torch.cuda.synchronize()
    return out, int(err.item())


def _spacing32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def _compare(host, park, N, idx):
    ac = _ac(N)
    rows = np.arange(len(host['natoms'])) if idx is None else np.asarray(idx)
    B = len(rows)
    out, err = _gather(park, N, host['natoms'], idx)
    assert err == 0
    assert all(g.intact() for g in out.values())
    parsed = (host['charges'][rows], host['bags'][rows], host['natoms'][rows], host['pos'][rows])
    placed = (host['acts'][rows], host['dev_plus'][rows], host['dev_minus'][rows], host['z_new'][rows])
    want = ac._assemble(parsed, placed)
    TA, MA, ME = gather_totals(host['natoms'][rows])
    assert (want.cfg.TA, want.cfg.MA, want.cfg.ME) == (TA, MA, ME)
    for k in ('mol_off', 'edge_off', 'molZ', 'molpos', 'bags', 'actions'):
        got, exp = out[k].t, getattr(want, k).reshape(-1)
        assert got.dtype == exp.dtype and got.shape == exp.shape and torch.equal(got, exp), k
    for k in ('logp', 'adv', 'ret'):
        assert torch.equal(out[k].t, torch.from_numpy(host[k][rows]).cuda()), k
    # the appended atoms: float32(mg_int_place) exactly (part of molpos above), and within one float32 spacing of
    # float32(place_new_atoms) -- the two float64 results differ by at most 1e-12, so their roundings are equal or adjacent
    mol_off = out['mol_off'].t.cpu().numpy()
    molpos = out['molpos'].t.cpu().numpy().reshape(MA, 3)
    for s, (dev, ref) in enumerate(((host['dev_plus'], host['ref_plus']), (host['dev_minus'], host['ref_minus'])), start=1):
        last = mol_off[s * B + 1:(s + 1) * B + 1] - 1
        got = molpos[last]
        assert np.array_equal(got, dev[rows].astype(np.float32))
        ref32 = ref[rows].astype(np.float32)
        assert np.all(np.abs(got.astype(np.float64) - ref32.astype(np.float64)) <= np.maximum(_spacing32(got), _spacing32(ref32)))
        assert np.abs(dev[rows] - ref[rows]).max() <= 1e-12


def _index_lists(S):
    rng = np.random.default_rng(17)
    return {'one': np.array([13]), 'subset': rng.permutation(S)[:23], 'replacement': rng.integers(0, S, size=257), 'identity': None}


@pytest.mark.parametrize('which', ['one', 'subset', 'replacement', 'identity'])
def test_canvas_9_equals_the_host_assembly(built_lib, which):
    """B = 1; a permuted subset; 257 rows drawn with replacement (the scan's 256-sample chunk carry); no index list"""
    host, park = _rollout9()
    idx = _index_lists(40)[which]
    if which == 'replacement':
        assert set(range(10, 17)) <= set(idx.tolist()) and {0, 1, 2, 3, 4} <= set(idx.tolist())  # the ties and n = 0, N, 1, 2, 3
    _compare(host, park, 9, idx)


def test_canvas_255_equals_the_host_assembly(built_lib):
    host, park = _rollout255()
    _compare(host, park, 255, None)


def _offsets_stay_inside(out, B, MA, ME):
    mol_off, edge_off = out['mol_off'].t.cpu().numpy().astype(np.int64), out['edge_off'].t.cpu().numpy().astype(np.int64)
    assert mol_off[0] == 0 and mol_off[3 * B] == MA and np.all(np.diff(mol_off) >= 0) and mol_off.min() >= 0 and mol_off.max() <= MA
    assert edge_off[0] == 0 and np.all(np.diff(edge_off) >= 0) and edge_off.min() >= 0 and edge_off.max() <= ME
    size = np.diff(mol_off)
    if edge_off[3 * B] < ME:  # (nothing was clamped: the pair offsets are the sizes')
        assert np.array_equal(np.diff(edge_off), size * (size - 1))
    for k in NAMES:  # every element was written
        raw = out[k].t.view(torch.int64) if out[k].t.dtype == torch.float64 else out[k].t.view(torch.int32)
        assert not bool((raw == -1).any()), k


def test_handled_bad_input(built_lib):
    host, park = _rollout9()
    idx = _index_lists(40)['subset']
    B = len(idx)
    TA, MA, ME = gather_totals(host['natoms'][idx])
    for off in (1, -1):  # the host's TA off by one: flag 1, a layout inside the sizes the host gave
        totals = (TA + off, MA + 3 * off, ME)
        out, err = _gather(park, 9, host['natoms'], idx, totals)
        assert err == 1 and all(g.intact() for g in out.values())
        _offsets_stay_inside(out, B, totals[1], ME)
        assert torch.equal(out['logp'].t, torch.from_numpy(host['logp'][idx]).cuda())
    out, err = _gather(park, 9, host['natoms'], idx, (TA, MA, ME + 2))
    assert err == 1 and all(g.intact() for g in out.values())
    _offsets_stay_inside(out, B, MA, ME + 2)
    # a count of N + 1 in the parked atom counts: flag 2
    bad = dict(park, s_natoms=park['s_natoms'].clone())
    bad['s_natoms'][int(idx[5])] = 10
    out, err = _gather(bad, 9, host['natoms'], idx)
    assert err == 2 and all(g.intact() for g in out.values())
    _offsets_stay_inside(out, B, MA, ME)
    # an index outside the rollout: flag 2
    wild = idx.copy()
    wild[3] = 40
    out, err = _gather(park, 9, np.append(host['natoms'], 0), wild)
    assert err == 2 and all(g.intact() for g in out.values())
    wild[3] = -1
    out, err = _gather(park, 9, np.append(host['natoms'], 0), wild)
    assert err == 2 and all(g.intact() for g in out.values())


def test_bad_arguments_launch_nothing(built_lib):
    host, park = _rollout9()
    idx = _index_lists(40)['subset']
    B = len(idx)
    totals = gather_totals(host['natoms'][idx])
    poison = torch.full((1 << 16, ), 0x5A, dtype=torch.uint8, device='cuda')
    out = {k: _Same(poison) for k in NAMES}
    idx_dev = torch.from_numpy(idx).cuda()
    call = lambda **kw: _call(park, kw.pop('N', 9), kw.pop('B', B), kw.pop('idx', idx_dev), kw.pop('totals', totals), out,
                              poison, **kw)
    for name in PARKED + NAMES + ('err', ):
        assert call(replace={name: None}) == EINVAL, name
    assert call(B=0) == EINVAL and call(B=-3) == EINVAL
    assert call(N=0) == EINVAL and call(N=256) == EINVAL
    assert call(Z=1) == EINVAL and call(Z=17) == EINVAL
    assert call(totals=(totals[0], totals[1] + 1, totals[2])) == EINVAL and call(totals=(totals[0] + 1, totals[1], totals[2])) == EINVAL
    assert call(idx=None, S=B - 1) == EINVAL and call(S=0) == EINVAL
    torch.cuda.synchronize()
    assert bool((poison == 0x5A).all())
