"""Every device-side draw of a rollout step, replayed on the host (tests/draw_ref.py): the draw kernels of sampling.inc and
int_sampling.inc decide which action is taken, and a draw from a slightly wrong distribution leaves logp / ent / v exactly right.
Here step_canvas(commit=False, seed, sample_ids) runs in both modes, the distribution parameters of the pass that drew are read
back from the workspace, the uniforms are recomputed from (seed, base + stride * row, stream, draw), and the float64 replay
must name the same action row by row -- except on rows whose uniform sits within the float32 margin of a decision boundary,
whose share is bounded.  Cases: the smallest shapes at which each kernel form can go wrong (a grid tail, empty / one-atom /
full canvases, bags with one element left, 9 and 16 symbols, the focus pick over 255 atoms, peaked and flat logits, one and
eight mixture components, both orientation families, keyed half-batches)."""
import ctypes as C

import numpy as np
import pytest
import torch

from molgym_amd import _lib
from molgym_amd.spaces import ActionSpace, ObservationSpace
from molgym_amd.synthetic import CONFIGS
from tests import draw_ref as D
from tests.helpers import make_pair

pytestmark = pytest.mark.gpu
ZS3 = [0, 9, 16]
ZS16 = [0, 1, 5, 6, 7, 8, 9, 14, 15, 16, 17, 33, 34, 35, 52, 53]
SEED = 0x2545F4914F6CDD1D
MODES = (D.TRAIN, D.EVAL)


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def _canvas(rng, n, N, Z):
    """synthetic.make_canvas's random walk (bonds U(1.10, 2.10), no pair closer than 0.6), the distance test vectorised"""
    pos = np.zeros((max(n, 1), 3))
    k = 0
    while k < n:
        if k:
            v = rng.normal(size=3)
            cand = pos[rng.integers(k)] + rng.uniform(1.10, 2.10) * v / np.linalg.norm(v)
            if np.min(np.linalg.norm(pos[:k] - cand, axis=1)) < 0.6:
                continue
            pos[k] = cand
        k += 1
    labels = rng.integers(1, Z, size=n)
    return tuple([(int(l), tuple(float(x) for x in p)) for l, p in zip(labels, pos[:n])] + [(0, (0.0, 0.0, 0.0))] * (N - n))


def _bag(rng, Z, kind):
    bag = np.zeros(Z, dtype=np.int64)
    real = np.arange(1, Z)
    if kind == 'single':            # one element left
        bag[rng.choice(real)] = 1
    elif kind == 'no_first':        # the first symbols zeroed
        bag[Z // 2:] = rng.integers(1, 4, size=Z - Z // 2)
    elif kind == 'no_last':
        bag[1:Z // 2] = rng.integers(1, 4, size=Z // 2 - 1)
    elif kind == 'alternating':
        bag[1::2] = rng.integers(1, 4, size=len(bag[1::2]))
    else:
        bag[1:] = rng.integers(0, 4, size=Z - 1)
        if bag.sum() == 0:
            bag[rng.choice(real)] = 2
    return tuple(int(x) for x in bag)


def _observations(B, N, Z, seed, counts=None, low=3, edges=True):
    """with `edges`, rows 0 / 1 / 2: an empty, a one-atom and a full canvas, row 3 two atoms when low < 3; the other canvases hold
    low .. N atoms.  Few rows sit below `low` because symmetry leaves the evaluation-mode draws of such canvases undecided: two
    atoms give an orientation density that is constant around the bond, up to three atoms give mirror-image placements
    for the two dihedral signs, whose kappa logits differ by rounding alone.  Every eighth bag has a single element left; above
    three symbols the others cycle through first / last / alternating symbols zeroed and random bags."""
    rng = np.random.default_rng(seed)
    if counts is None:
        counts = rng.integers(low, N + 1, size=B)
        if edges:
            counts[:3] = (0, 1, N)
            if low <= 3:
                counts[3] = 2
    kinds = ('single', 'no_first', 'no_last', 'alternating', 'random', 'random', 'single', 'random')
    return [(_canvas(rng, int(n), N, Z), _bag(rng, Z, kinds[b % len(kinds)] if Z > 3 or b % 4 == 0 else 'random'))
            for b, n in enumerate(counts)]


def _scale_heads(ac, factor):
    """the last Linear of the focus and element heads times `factor` (30: most of the mass on one entry, the max subtraction
    matters; 0: a flat distribution of bit-identical logits)"""
    with torch.no_grad():
        for head in ('phi_focus', 'phi_element'):
            for part in ('weight', 'bias'):
                off, shape = ac.slot_table[f'{head}.layers.1.{part}']
                ac.theta[off:off + int(np.prod(shape))] *= factor


class _Pool:
    """rows of several calls of one case, checked together: (got, want, ambiguous) per sub-action"""

    def __init__(self, case):
        self.case, self.parts = case, {}

    def add(self, name, got, want, amb):
        self.parts.setdefault(name, []).append((np.asarray(got), np.asarray(want), np.asarray(amb)))

    def check(self, caps):
        for name, rows in self.parts.items():
            got, want, amb = (np.concatenate([r[i] for r in rows]) for i in range(3))
            share, n = D.check(got, want, amb, caps[name], f'{self.case} {name}')
            print(f'draws[{self.case}] {name}: ambiguous share {share:.4f}, {n} rows compared')


# ---- CovariantAC ------------------------------------------------------------------------------------------------------------
def _cov_agent(monkeypatch, zs, N, seed, beta=1.0, **kw):
    name = f'draws{len(zs)}_{N}'
    monkeypatch.setitem(CONFIGS, name, dict(zs=zs, canvas_size=N, batch=16, bag_scale=20 if N > 7 else 5, beta=beta))
    ac, _, _ = make_pair(name, seed=seed, **kw)
    return ac


def _cov_replay(pool, ac, obs, seed, ids, mode):
    ac.training = mode == D.TRAIN
    cv = ac.make_canvas(obs)
    with torch.no_grad():
        out = ac.step_canvas(cv, commit=False, seed=seed, sample_ids=ids)
    B, N, Z, G, CE = len(obs), cv.N, len(ac.zs), ac.num_gaussians, ac.num_channels_per_element
    blk = out['dists']._block.cpu().numpy()
    a = out['a'].cpu().numpy()
    cut = np.cumsum([0, B * N, B, B * Z, B * 2 * G, B * 25 * CE * 2, B])
    logit_f, natoms, logit_e, dout, coef, _ = (blk[cut[i]:cut[i + 1]] for i in range(6))
    natoms = np.rint(natoms).astype(np.int64)
    assert np.array_equal(natoms, cv.natoms)
    s = D.samples_of(ids[0], ids[1], B)
    length = np.maximum(natoms, 1)
    want, amb = D.categorical(logit_f.reshape(B, N), np.arange(N)[None, :] < length[:, None], D.u01(seed, s, 0, 0), mode, length)
    pool.add('focus', a[:, 0], want, amb)
    bags = np.array([o[1] for o in obs])
    want, amb = D.categorical(logit_e.reshape(B, Z), bags > 0, D.u01(seed, s, 1, 0), mode)
    pool.add('element', a[:, 1], want, amb)
    off, _ = ac.slot_table['distance_log_stds']
    logstd = ac.theta.detach()[off:off + G].cpu().numpy()
    lo, hi = np.float32(ac.min_distance), np.float32(ac.max_distance)
    half_w, center = (hi - lo) / np.float32(2), (hi + lo) / np.float32(2)
    if mode == D.TRAIN:
        want, amb = D.gmm(dout.reshape(B, 2 * G), logstd, G, half_w, center, *(D.u01(seed, s, 2, j) for j in range(3)))
        assert want.min() >= 0.001
    else:
        want, amb = D.gmm_best_of(dout.reshape(B, 2 * G), logstd, G, half_w, center, seed, s)
    pool.add('distance', a[:, 2], want, amb)
    has_beta = ac.beta is not None
    want, amb = D.so3_reject(coef.reshape(B, 25, CE, 2), has_beta, ac.beta, natoms == 0, seed, s, mode)
    pool.add('orientation', a[:, 3:6], want, amb)


def _cov_caps(mode):
    best = D.CAP_BEST_OF if mode == D.EVAL else None
    return {'focus': D.CAP_CATEGORICAL, 'element': D.CAP_CATEGORICAL, 'distance': best or D.CAP_CATEGORICAL,
            'orientation': best or D.CAP_SO3_TRAIN}


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('beta,G,ids', [(1.0, 1, (0, 1)), (None, 8, (0, 1)), (1.0, 8, (3, 5)), (None, 1, (0, 1))])
def test_covariant_canvas7_grid_tail(built_lib, monkeypatch, beta, G, ids, mode):
    """B = 70: the one-thread-per-row kernels launch 64-wide blocks, six rows sit in the tail block"""
    ac = _cov_agent(monkeypatch, ZS3, 7, seed=41, beta=beta, num_gaussians=G)
    pool = _Pool(f'cov c7 beta={beta} G={G} ids={ids} mode={mode}')
    for k in range(2):
        _cov_replay(pool, ac, _observations(70, 7, 3, seed=50 + k), SEED + k, ids, mode)
    pool.check(_cov_caps(mode))


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('Z', [9, 16])
def test_covariant_wide_element_sets(built_lib, monkeypatch, Z, mode):
    """k_sample_element<true>: the bag mask over 9 / 16 symbols, bags zero at the first, the last, alternating symbols"""
    ac = _cov_agent(monkeypatch, ZS16[:Z], 7, seed=42)
    pool = _Pool(f'cov Z={Z} mode={mode}')
    for k in range(6):
        _cov_replay(pool, ac, _observations(24, 7, Z, seed=60 + k, edges=k == 0), SEED + 10 + k, (0, 1), mode)
    pool.check(_cov_caps(mode))


@pytest.mark.parametrize('mode', MODES)
def test_covariant_canvas255_focus_pick(built_lib, monkeypatch, mode):
    """rows of 0, 1, 64 and 255 atoms: the focus pick walks the staged heads' logits, up to 255 of them"""
    ac = _cov_agent(monkeypatch, [0, 1, 6, 7, 8], 255, seed=43)
    obs = _observations(4, 255, 5, seed=70, counts=[0, 1, 64, 255])
    pool = _Pool(f'cov c255 mode={mode}')
    for k in range(16):
        _cov_replay(pool, ac, obs, SEED + 20 + k, (k, 3), mode)
    pool.check(_cov_caps(mode))


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('factor', [30.0, 0.0])
def test_covariant_peaked_and_flat_heads(built_lib, monkeypatch, factor, mode):
    ac = _cov_agent(monkeypatch, ZS3, 7, seed=44)
    _scale_heads(ac, factor)
    pool = _Pool(f'cov heads x{factor:g} mode={mode}')
    for k in range(2):
        _cov_replay(pool, ac, _observations(70, 7, 3, seed=80 + k), SEED + 40 + k, (0, 1), mode)
    pool.check(_cov_caps(mode))


@pytest.mark.parametrize('mode', MODES)
def test_covariant_keyed_half_batches(built_lib, monkeypatch, mode):
    """group g of 2 holds the rows g, g + 2, ...: replayed with the keys (g, 2), and equal to the full launch's rows"""
    ac = _cov_agent(monkeypatch, ZS3, 7, seed=45)
    obs = _observations(70, 7, 3, seed=90)
    pool = _Pool(f'cov halves mode={mode}')
    for g in range(2):
        _cov_replay(pool, ac, obs[g::2], SEED + 50, (g, 2), mode)
    _cov_replay(pool, ac, obs, SEED + 50, (0, 1), mode)
    pool.check(_cov_caps(mode))
    for name, rows in pool.parts.items():
        for g in range(2):
            assert np.array_equal(rows[g][0], rows[2][0][g::2]), name


# ---- SchNetAC ---------------------------------------------------------------------------------------------------------------
def _int_agent(zs, N, seed, width=64):
    from molgym_amd.agents.internal import SchNetAC
    torch.manual_seed(seed)
    ac = SchNetAC(ObservationSpace(N, zs), ActionSpace(zs), (0.8, 1.8), width, device='cuda:0')
    with torch.no_grad():  # non-zero biases: every head depends on its inputs
        g = torch.Generator().manual_seed(seed + 1)
        for name, (off, shape) in ac.slot_table.items():
            n = int(np.prod(shape))
            if name.endswith('bias'):
                ac.theta[off:off + n] = (0.1 * torch.randn(n, generator=g)).to(ac.theta)
    return ac


def _place_dev(cv, acts):
    """mg_int_place: both z-matrix placements (dihedral kept / flipped) of completed action rows"""
    B, N = cv.E, cv.N
    dev = cv.pos64.device
    a = torch.from_numpy(np.ascontiguousarray(acts, dtype=np.float32)).to(dev)
    plus = torch.empty(B, 3, dtype=torch.float64, device=dev)
    minus = torch.empty_like(plus)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().mg_int_place(B, N, ptr(cv.pos64), ptr(cv.natoms_dev), ptr(a), ptr(plus), ptr(minus),
                                           C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return plus.cpu().numpy(), minus.cpu().numpy()


def _int_replay(pool, ac, obs, seed, ids, mode):
    ac.training = mode == D.TRAIN
    cv = ac.make_canvas(obs)
    with torch.no_grad():
        out = ac.step_canvas(cv, commit=False, seed=seed, sample_ids=ids)
    cfg, ws = ac._last_sample_cfg, ac._last_ws
    B, N, Z = len(obs), cv.N, len(ac.zs)
    a = out['a'].cpu().numpy()
    view = lambda name, cnt: ac._ws_view(cfg, ws, name)[:cnt].cpu().numpy()
    natoms = cv.natoms.astype(np.int64)
    s = D.samples_of(ids[0], ids[1], B)
    assert np.all(a[:, 0] == 0)
    ragged = view('logitF', int(natoms.sum()))
    logit_f = np.zeros((B, N), dtype=np.float32)
    real = np.arange(N)[None, :] < natoms[:, None]
    logit_f[real] = ragged                       # (row-major: the atoms of row 0 first, as the base molecules lie)
    length = np.maximum(natoms, 1)
    want, amb = D.categorical(logit_f, np.arange(N)[None, :] < length[:, None], D.u01(seed, s, 0, 0), mode, length)
    pool.add('focus', a[:, 1], want, amb)
    bags = np.array([o[1] for o in obs])
    want, amb = D.categorical(view('logitE', B * Z).reshape(B, Z), bags > 0, D.u01(seed, s, 1, 0), mode)
    pool.add('element', a[:, 2], want, amb)
    off, _ = ac.slot_table['log_stds']
    par = np.array(list(ac._draw_par()), dtype=np.float32)
    want, amb = D.normal3(view('cout', B * 3).reshape(B, 3), ac.theta.detach()[off:off + 3].cpu().numpy(), par[:3], par[3:],
                          D.normal3_uniforms(seed, s), mode)
    assert want[:, 0].min() >= 0.001
    pool.add('continuous', a[:, 3:6], want, amb)
    kappa, amb = D.categorical(view('kv', 2 * B).reshape(2, B).T, np.ones((B, 2), dtype=bool), D.u01(seed, s, 3, 0), mode)
    pool.add('kappa', a[:, 6], kappa, amb)
    # rows 0 / 1 of kappa swap the position taken from `place`: newpos is the replayed choice of the two placements of the row
    plus, minus = _place_dev(cv, a)
    newpos = np.array([p for _, p in out['actions']])
    off_by = np.abs(newpos - np.where(kappa[:, None] == 1, minus, plus)).max(axis=1)
    assert np.all(amb | (off_by <= 1e-12)), (pool.case, np.nonzero(~amb & ~(off_by <= 1e-12))[0])


INT_CAPS = {'focus': D.CAP_CATEGORICAL, 'element': D.CAP_CATEGORICAL, 'continuous': 0.0, 'kappa': D.CAP_CATEGORICAL}


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('ids', [(0, 1), (3, 5)])
def test_internal_canvas7_grid_tail(built_lib, ids, mode):
    ac = _int_agent(ZS3, 7, seed=51)
    pool = _Pool(f'int c7 ids={ids} mode={mode}')
    for k in range(2):
        _int_replay(pool, ac, _observations(70, 7, 3, seed=100 + k, low=4), SEED + 60 + k, ids, mode)
    pool.check(INT_CAPS)


@pytest.mark.parametrize('mode', MODES)
def test_internal_canvas20_grouped_heads(built_lib, mode):
    ac = _int_agent(ZS3, 20, seed=52)
    pool = _Pool(f'int c20 mode={mode}')
    for k in range(2):
        _int_replay(pool, ac, _observations(70, 20, 3, seed=110 + k, low=4), SEED + 70 + k, (0, 1), mode)
    pool.check(INT_CAPS)


@pytest.mark.parametrize('mode', MODES)
def test_internal_canvas255_focus_pick(built_lib, mode):
    ac = _int_agent([0, 1, 6, 7, 8], 255, seed=53)
    obs = _observations(4, 255, 5, seed=120, counts=[0, 1, 255, 64])
    pool = _Pool(f'int c255 mode={mode}')
    for k in range(16):
        _int_replay(pool, ac, obs, SEED + 80 + k, (k, 3), mode)
    pool.check(INT_CAPS)


@pytest.mark.parametrize('mode', MODES)
def test_internal_sixteen_symbols(built_lib, mode):
    ac = _int_agent(ZS16, 7, seed=54)
    pool = _Pool(f'int Z=16 mode={mode}')
    for k in range(6):
        _int_replay(pool, ac, _observations(24, 7, 16, seed=130 + k, low=4, edges=k == 0), SEED + 100 + k, (0, 1), mode)
    pool.check(INT_CAPS)


@pytest.mark.parametrize('mode', MODES)
def test_internal_keyed_half_batches(built_lib, mode):
    ac = _int_agent(ZS3, 7, seed=55)
    obs = _observations(70, 7, 3, seed=140, low=4)
    pool = _Pool(f'int halves mode={mode}')
    for g in range(2):
        _int_replay(pool, ac, obs[g::2], SEED + 110, (g, 2), mode)
    _int_replay(pool, ac, obs, SEED + 110, (0, 1), mode)
    pool.check(INT_CAPS)
    for name, rows in pool.parts.items():
        for g in range(2):
            assert np.array_equal(rows[g][0], rows[2][0][g::2]), name
