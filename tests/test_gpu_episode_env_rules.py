"""mg_episode_step_rules / mg_episode_draw_formulas against the host statement of their rules (tests/episode_rules_ref.py):
every output and state array compared exactly, between guard bands, slots beyond natoms poisoned (the tables of
tests/test_gpu_episode_rules.py plant the candidate's own position and a carbon there)."""
import ctypes as C

import numpy as np
import pytest
import torch

from molgym_amd import _lib
from tests import episode_ref as R
from tests import episode_rules_ref as X
from tests import test_gpu_episode_rules as B

pytestmark = pytest.mark.gpu
DEV = B.DEV
MIN_D, MAX_SOLO, GUARD = B.MIN_D, B.MAX_SOLO, B.GUARD
ZS5 = B.ZS5  # [0, 1, 6, 17, 35]
ZSF = [0, 1, 6, 7, 8]  # every element has a bond count
CUBE = np.array([(1, 0, 0, -1), (-1, 0, 0, 0), (0, 1, 0, -1), (0, -1, 0, 0), (0, 0, 1, -1), (0, 0, -1, 0)], dtype=np.float64)  # [0, 1]^3


def _stream():
    return C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)


def _rules(dev, ptr, num_refills=0, planes=None, hull_tol=0.0, sampler=None):
    r = _lib.EpisodeRules()
    r.num_refills, r.hull_tol = num_refills, hull_tol
    r.refills, r.formula_no = ptr('refills').value, ptr('formula_no').value
    if planes is not None:
        r.num_planes, r.planes = len(planes), ptr('planes').value
    if sampler is not None:
        r.stochastic, r.size_min, r.size_max, r.max_tries = 1, sampler['size_min'], sampler['size_max'], sampler['max_tries']
        r.seed, r.stream_base, r.stream_stride = sampler['seed'], sampler['base'], sampler['stride']
        for i, c in enumerate(sampler['counts']):
            r.counts[i] = int(c)
    return r


def _with_counters(st, refills=0, formula_no=None):
    E = st['natoms'].shape[0]
    st = dict(st)
    st['refills'] = np.broadcast_to(np.asarray(refills, dtype=np.int32), (E, )).copy()
    st['formula_no'] = st['episode_no'].copy() if formula_no is None else np.broadcast_to(np.asarray(formula_no, dtype=np.int32), (E, )).copy()
    return st


def device_step(st, zs, actions, newpos, compute_pos, min_d=MIN_D, max_solo=MAX_SOLO, num_refills=0, planes=None, hull_tol=0.0,
                sampler=None):
    """one mg_episode_step_rules launch on copies of the arrays: every array after, guard bands checked"""
    E, N = st['charges'].shape
    Z, F = st['bags'].shape[1], st['formulas'].shape[0]
    host = dict(st, actions=np.asarray(actions, dtype=np.float32), newpos=np.asarray(newpos, dtype=np.float64),
                status=np.full(E, -99, dtype=np.int32), element=np.full(E, -99, dtype=np.int32))
    if planes is not None:
        host['planes'] = np.asarray(planes, dtype=np.float64)
    dev = {k: B._guarded(v) for k, v in host.items()}
    ptr = lambda k: C.c_void_p(dev[k].data_ptr() + GUARD * dev[k].element_size())
    rules = _rules(dev, ptr, num_refills, planes, hull_tol, sampler)
    with torch.cuda.device(DEV):
        _lib.check(_lib.lib().mg_episode_step_rules(E, N, Z, F, host['actions'].shape[1], int(compute_pos), (C.c_int32 * Z)(*zs), min_d,
                                                    max_solo, ptr('actions'), ptr('newpos'), ptr('pos64'), ptr('pos32'), ptr('charges'),
                                                    ptr('bags'), ptr('natoms'), ptr('alive'), ptr('episode_no'), ptr('start_pos64'),
                                                    ptr('start_charges'), ptr('start_natoms'), ptr('formulas'), ptr('status'),
                                                    ptr('element'), C.byref(rules), _stream()))
        torch.cuda.synchronize()
    got = {}
    for k, t in dev.items():
        flat = t.cpu().numpy()
        band = B._poison(flat.dtype)
        assert np.all(flat[:GUARD] == band) and np.all(flat[-GUARD:] == band), f'guard band of {k} overwritten'
        got[k] = flat[GUARD:-GUARD].reshape(host[k].shape)
    return got


def check_against_model(st, zs, actions, newpos, compute_pos, min_d=MIN_D, max_solo=MAX_SOLO, **rules):
    got = device_step(st, zs, actions, newpos, compute_pos, min_d, max_solo, **rules)
    want = {k: v.copy() for k, v in st.items()}
    want_pos = np.array(newpos, dtype=np.float64)
    status, element = X.episode_step_rules(want, zs, np.asarray(actions, dtype=np.float32), want_pos, min_d, max_solo, compute_pos, **rules)
    want.update(status=status, element=element, newpos=want_pos, actions=np.asarray(actions, dtype=np.float32))
    if rules.get('planes') is not None:
        want['planes'] = np.asarray(rules['planes'], dtype=np.float64)
    assert set(want) == set(got)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    return status, got


def _random_actions(rng, E, zs, cols, N):
    acts = np.zeros((E, cols), dtype=np.float32)
    el = rng.integers(0, len(zs), size=E)
    acts[:, 1 if cols == 6 else 2] = np.where(rng.random(E) < 0.05, rng.choice([-1, len(zs)], size=E), el)
    if cols == 6:
        acts[:, 0] = rng.integers(0, N, size=E)
        acts[:, 2] = rng.uniform(0.2, 2.0, size=E)
        d = rng.normal(size=(E, 3))
        acts[:, 3:6] = d / np.linalg.norm(d, axis=1, keepdims=True)
    return acts, el


@pytest.mark.parametrize('cols', [7, 6])
def test_all_extras_off_equals_mg_episode_step(built_lib, cols):
    rng = np.random.default_rng(300 + cols)
    E, N, zs, F = 500, 12, ZS5, 3
    st = B._random_state(rng, E, N, zs, F)
    acts, el = _random_actions(rng, E, zs, cols, N)
    newpos = rng.uniform(-1.75, 1.75, size=(E, 3))
    last = np.nonzero(rng.random(E) < 0.1)[0]
    st['bags'][last] = 0.0
    st['bags'][last, el[last]] = 1.0
    old = B.device_step(st, zs, acts, newpos, compute_pos=cols == 6)
    status, new = check_against_model(_with_counters(st), zs, acts, newpos, compute_pos=cols == 6)
    for k in old:
        assert np.array_equal(old[k], new[k]), k
    assert np.array_equal(new['formula_no'], new['episode_no']) and not new['refills'].any()
    assert np.all(np.bincount(status, minlength=8) >= 1) and status.max() < 8


def _hull_table(N=5):
    return B.Table(N, ZS5, [(0, 2, 1, 1, 0)])


def test_hull_faces_to_the_ulp(built_lib):
    """unit cube: a coordinate exactly on a face is inside, one ulp beyond is outside; hull_tol moves the face exactly"""
    for tol in (0.0, 0.25):
        t = _hull_table()
        hi = 1.0 + tol  # (1.25 - 1 is exact)
        for axis in range(3):
            for v, want in ((hi, R.PLACED), (np.nextafter(hi, 2.0), X.OUTSIDE), (np.nextafter(hi, 0.0), R.PLACED),
                            (-tol, R.PLACED), (np.nextafter(-tol, -1.0), X.OUTSIDE), (np.nextafter(-tol, 1.0), R.PLACED)):
                q = [0.5, 0.5, 0.5]
                q[axis] = v
                t.add([], 6, q, want)
                t.add([(6, (2.5, 2.5, 2.5))], 6, q, want)  # (an atom well away: only the hull decides)
        C0 = [(6, (1.25, 0.5, 0.5))]
        t.add(C0, 6, (1.5, 0.5, 0.5), X.OUTSIDE)  # also too close: the hull comes first (environment.py:159-164)
        t.add(C0, 6, (0.875, 0.5, 0.5), R.TOO_CLOSE)  # inside, and too close
        t.add([(17, (0.5, 0.5, 0.5))], 1, (0.5, 0.5, 1.75), X.OUTSIDE)  # also solo
        t.add(C0, 0, (7.0, 7.0, 7.0), R.STOP)  # a stop is not a position
        t.add([], 0, (-3.0, 0.0, 0.0), R.STOP)
        t.add(C0, 6, (7.0, 7.0, 7.0), R.INACTIVE, alive=0)
        t.add(C0, 6, (7.0, 7.0, 7.0), R.ERROR, element=9)  # the error checks come first
        st, acts, newpos = t.arrays()
        assert R.decide(ZS5, 5, [6], np.array([C0[0][1]]), [0, 3, 3, 3, 3], 2, np.array((1.5, 0.5, 0.5)), MIN_D, MAX_SOLO) == R.TOO_CLOSE
        status, got = check_against_model(_with_counters(st), ZS5, acts, newpos, False, planes=CUBE, hull_tol=tol)
        assert list(status) == t.expect
        outside = status == X.OUTSIDE
        assert np.array_equal(got['natoms'][outside], st['start_natoms'][outside]) and np.all(got['episode_no'][outside] == 1)


def _deciding_points(points, deciding):
    """per facet k of the Fibonacci scaffold: a point 1e-4 beyond its centroid (outside by plane k ALONE) and one 1e-4 inside"""
    from scipy.spatial import ConvexHull
    pts = X.fibonacci_sphere(points, 3.0)
    hull, planes = ConvexHull(pts), X.hull_planes(pts)
    assert np.array_equal(hull.equations, planes)
    cases = []
    for k in deciding:
        centroid = pts[hull.simplices[k]].mean(axis=0)
        for step, want in ((1e-4, X.OUTSIDE), (-1e-4, R.PLACED)):
            q = centroid + step * planes[k, :3]
            vals = X.hull_values(planes, q)
            assert int(np.argmax(vals)) == k and int((vals > 0).sum()) == (1 if want == X.OUTSIDE else 0), (k, vals.max())
            cases.append((q, want))
    return planes, cases


@pytest.mark.parametrize('points,num_planes,deciding', [(35, 66, (0, 63, 64, 65)), (34, 64, (63, ))])
def test_hull_deciding_plane_in_every_lane_round(built_lib, points, num_planes, deciding):
    """lanes stride over the planes: the ONE violated plane in the first lane, the last lane and the second round"""
    planes, cases = _deciding_points(points, deciding)
    assert planes.shape == (num_planes, 4)
    t = _hull_table()
    for q, want in cases:
        t.add([], 6, q, want)
    t.add([], 6, (0.0, 0.0, 0.0), R.PLACED)
    st, acts, newpos = t.arrays()
    status, _ = check_against_model(_with_counters(st), ZS5, acts, newpos, False, planes=planes)
    assert list(status) == t.expect


@pytest.mark.parametrize('N', [3, 6])
def test_refills(built_lib, N):
    zs, F = ZS5, 2
    formulas = [(0, 2, 1, 1, 0), (0, 0, 2, 0, 1)]
    one_c = [0.0, 0.0, 1.0, 0.0, 0.0]
    t = B.Table(N, zs, formulas)
    refills, fno = [], []

    def add(*a, r=0, f=0, **kw):
        t.add(*a, **kw)
        refills.append(r)
        fno.append(f)

    near = [(6, (0.0, 0.0, 0.0))]
    add(near, 6, (1.0, 0, 0), X.REFILLED, bag=one_c, r=0, f=0)  # the bag empties with a refill left
    add(near, 6, (1.0, 0, 0), X.REFILLED, bag=one_c, r=0, f=1)  # formula_no wraps: (1 + 1) % 2
    add(near, 6, (1.0, 0, 0), X.REFILLED, bag=one_c, r=0, f=7)
    add(near, 6, (1.0, 0, 0), R.BAG_EMPTY, bag=one_c, r=1, f=1)  # none left
    add(B._far(N - 1), 6, (0, 0, 0), R.FULL, bag=one_c, r=0, f=0)  # the canvas fills: FULL, no refill consumed
    add(B._far(N - 1), 6, (0, 0, 0), R.FULL, bag=one_c, r=1, f=4)
    add(near, 6, (1.0, 0, 0), R.PLACED, r=1, f=3)  # a placement leaves the counters alone
    # refills is back to 0 after every kind of ending
    add(near, 0, (0, 0, 0), R.STOP, r=1, f=1)
    add(near, 6, (0.25, 0, 0), R.TOO_CLOSE, r=1, f=2)
    add(near, 1, (0, MAX_SOLO, 0), R.SOLO, r=1, f=3)
    add(near, 6, (1.0, 0.5, 9.0), X.OUTSIDE, r=1, f=4)
    add(near, 6, (1.0, 0, 0), R.ERROR, r=1, f=2, element=7)
    add(near, 6, (1.0, 0, 0), R.INACTIVE, r=1, f=2, alive=0)
    st, acts, newpos = t.arrays()
    st = _with_counters(st, refills, fno)
    planes = CUBE * np.array([1, 1, 1, 1.0]) + np.array([0, 0, 0, -4.0])  # the cube grown by 4 on every side: only z = 9 is outside
    status, got = check_against_model(st, zs, acts, newpos, False, num_refills=1, planes=planes)
    assert list(status) == t.expect
    ended = np.isin(status, X.DONE)
    assert ended.sum() == 7 and not got['refills'][ended].any()
    assert np.array_equal(got['formula_no'][ended], np.array(fno)[ended] + 1)
    assert list(got['refills'][:3]) == [1, 1, 1] and list(got['formula_no'][:3]) == [1, 2, 8]
    assert np.array_equal(got['bags'][:3], np.array([formulas[1], formulas[0], formulas[0]], dtype=np.float32))
    assert np.array_equal(got['natoms'][:3], st['natoms'][:3] + 1) and not got['episode_no'][:3].any()
    # the same rows without refills to give: every REFILLED is a BAG_EMPTY
    status0, _ = check_against_model(st, zs, acts, newpos, False, num_refills=0, planes=planes)
    assert list(status0) == [R.BAG_EMPTY if s == X.REFILLED else s for s in t.expect]


def _sampler(max_tries, seed=77, base=0, stride=1):
    return dict(counts=(0, 4, 1, 0, 1), size_min=2, size_max=7, max_tries=max_tries, seed=seed, base=base, stride=stride)  # C1 H4 O1


@pytest.mark.parametrize('cols', [7, 6])
def test_sampled_formulas_equal_the_host_replay(built_lib, cols):
    """E = 70: 18 workgroups of four waves, the last one half empty; every ending draws the bag the host replays"""
    rng = np.random.default_rng(500 + cols)
    E, N, zs = 70, 6, ZSF
    st = B._random_state(rng, E, N, zs, 1)
    acts, _ = _random_actions(rng, E, zs, cols, N)
    acts[::3, 1 if cols == 6 else 2] = 0.0  # every third row stops: enough endings whatever the random rows do
    newpos = rng.uniform(-1.75, 1.75, size=(E, 3))
    sampler = _sampler(64, seed=2**63 + 12345, base=3, stride=2)
    status, got = check_against_model(_with_counters(st), zs, acts, newpos, cols == 6, sampler=sampler)
    ended = np.isin(status, X.DONE)
    assert ended.sum() >= 20
    bags = {tuple(b) for b in got['bags'][ended]}
    assert len(bags) >= 5  # (not one bag over and over)
    for e in np.nonzero(ended)[0]:
        assert np.array_equal(got['bags'][e], X.draw_formula(sampler['counts'], zs, 2, 7, 64, sampler['seed'], 3 + 2 * e))
    # a fixed size: size_min == size_max
    fixed = dict(sampler, size_min=4, size_max=4)
    status, got = check_against_model(_with_counters(st), zs, acts, newpos, cols == 6, sampler=fixed)
    assert np.all(got['bags'][np.isin(status, X.DONE)].sum(axis=1) == 4)


def test_exhausted_tries_stop_the_row(built_lib):
    """max_tries = 1 and a formula that is valid about every second time: exactly the rows whose first try is invalid get
    ERROR and alive = 0, with nothing else of the row written"""
    rng = np.random.default_rng(9)
    E, N, zs = 70, 6, ZSF
    st = B._random_state(rng, E, N, zs, 1)
    st['alive'][:] = 1
    acts = np.zeros((E, 7), dtype=np.float32)  # every row stops
    sampler = _sampler(1)
    _, valid, _ = X.formula_tries(sampler['counts'], zs, 2, 7, sampler['seed'], np.arange(E), 0)
    assert 20 <= valid.sum() <= 50
    status, got = check_against_model(_with_counters(st), zs, acts, np.zeros((E, 3)), False, sampler=sampler)
    assert np.array_equal(status == R.ERROR, ~valid) and np.array_equal(status == R.STOP, valid)
    assert np.array_equal(got['alive'] == 0, ~valid)
    for k in ('pos64', 'charges', 'bags', 'natoms', 'episode_no', 'formula_no'):
        assert np.array_equal(got[k][~valid], st[k][~valid] if k in st else st['episode_no'][~valid]), k


def _draw(E, Z, zs, sampler, bags0):
    dev = dict(bags=B._guarded(bags0), ok=B._guarded(np.full(E, -5, dtype=np.int32)), refills=B._guarded(np.zeros(1, dtype=np.int32)),
               formula_no=B._guarded(np.zeros(1, dtype=np.int32)))
    ptr = lambda k: C.c_void_p(dev[k].data_ptr() + GUARD * dev[k].element_size())
    rules = _rules(dev, ptr, sampler=sampler)
    with torch.cuda.device(DEV):
        _lib.check(_lib.lib().mg_episode_draw_formulas(E, Z, (C.c_int32 * Z)(*zs), C.byref(rules), ptr('bags'), ptr('ok'), _stream()))
        torch.cuda.synchronize()
    out = {}
    for k in ('bags', 'ok'):
        flat = dev[k].cpu().numpy()
        band = B._poison(flat.dtype)
        assert np.all(flat[:GUARD] == band) and np.all(flat[-GUARD:] == band), f'guard band of {k} overwritten'
        out[k] = flat[GUARD:-GUARD]
    return out['bags'].reshape(E, Z), out['ok']


def test_draw_formulas_equal_the_replay(built_lib):
    E, zs = 70, ZSF
    Z = len(zs)
    bags0 = np.full((E, Z), -3.0, dtype=np.float32)
    sampler = _sampler(64, seed=5, base=1, stride=3)
    bags, ok = _draw(E, Z, zs, sampler, bags0)
    want = np.array([X.draw_formula(sampler['counts'], zs, 2, 7, 64, 5, 1 + 3 * e) for e in range(E)], dtype=np.float32)
    assert np.all(ok == 1) and np.array_equal(bags, want)
    sampler = _sampler(1, seed=5)
    first, valid, _ = X.formula_tries(sampler['counts'], zs, 2, 7, 5, np.arange(E), 0)
    bags, ok = _draw(E, Z, zs, sampler, bags0)
    assert 0 < valid.sum() < E and np.array_equal(ok == 1, valid)
    assert np.array_equal(bags[valid], first[valid].astype(np.float32)) and np.all(bags[~valid] == -3.0)
    # the largest formula: 255 symbols, four a lane
    big = dict(counts=(0, 3, 2, 1, 2), size_min=255, size_max=255, max_tries=64, seed=11, base=0, stride=1)
    bags, ok = _draw(6, Z, zs, big, np.zeros((6, Z), dtype=np.float32))
    want = np.array([X.draw_formula(big['counts'], zs, 255, 255, 64, 11, e) for e in range(6)], dtype=np.float32)
    assert np.all(ok == 1) and np.array_equal(bags, want) and np.all(bags.sum(axis=1) == 255)


def test_bad_arguments_are_refused(built_lib):
    """every call is made on valid arrays, so only the named argument can be what is refused (and nothing is launched)"""
    rng = np.random.default_rng(1)
    E, N, zs = 4, 5, ZSF
    Z = len(zs)
    st = _with_counters(B._random_state(rng, E, N, zs, 1))
    host = dict(st, actions=np.zeros((E, 7), dtype=np.float32), newpos=np.zeros((E, 3)), status=np.zeros(E, dtype=np.int32),
                element=np.zeros(E, dtype=np.int32), planes=CUBE, ok=np.zeros(E, dtype=np.int32))
    dev = {k: B._guarded(v) for k, v in host.items()}
    ptr = lambda k: C.c_void_p(dev[k].data_ptr() + GUARD * dev[k].element_size())
    zs_c = (C.c_int32 * Z)(*zs)

    def step(rules):
        return _lib.lib().mg_episode_step_rules(E, N, Z, 1, 7, 0, zs_c, MIN_D, MAX_SOLO, ptr('actions'), ptr('newpos'), ptr('pos64'),
                                                ptr('pos32'), ptr('charges'), ptr('bags'), ptr('natoms'), ptr('alive'), ptr('episode_no'),
                                                ptr('start_pos64'), ptr('start_charges'), ptr('start_natoms'), ptr('formulas'),
                                                ptr('status'), ptr('element'), rules, _stream())

    def edited(base, **kw):
        r = _rules(dev, ptr, **base)
        for k, v in kw.items():
            setattr(r, k, v)
        return C.byref(r)

    sampled, hull = dict(sampler=_sampler(64)), dict(planes=CUBE)
    EINVAL = -1
    with torch.cuda.device(DEV):
        assert step(None) == EINVAL  # no rules at all
        for base, kw in ((sampled, dict(max_tries=0)), (sampled, dict(max_tries=65)), (sampled, dict(size_min=8, size_max=7)),
                         (sampled, dict(size_min=0)), (sampled, dict(size_max=256)), (sampled, dict(num_refills=1)),
                         (hull, dict(num_planes=-1)), (hull, dict(num_planes=511)), (hull, dict(planes=None)),
                         (hull, dict(hull_tol=-0.5)), ({}, dict(num_refills=-1)), ({}, dict(refills=None)), ({}, dict(formula_no=None))):
            assert step(edited(base, **kw)) == EINVAL, kw
            assert _lib.lib().mg_last_error()
        no_bond = _rules(dev, ptr, sampler=dict(_sampler(64), counts=(0, 1, 1, 1, 1)))
        zs_s = (C.c_int32 * Z)(0, 1, 6, 16, 8)  # sulfur has no bond count
        args = [ptr(k) for k in ('actions', 'newpos', 'pos64', 'pos32', 'charges', 'bags', 'natoms', 'alive', 'episode_no', 'start_pos64',
                                 'start_charges', 'start_natoms', 'formulas', 'status', 'element')]
        assert _lib.lib().mg_episode_step_rules(E, N, Z, 1, 7, 0, zs_s, MIN_D, MAX_SOLO, *args, C.byref(no_bond), _stream()) == EINVAL
        assert step(edited(sampled, counts=(C.c_int32 * 16)())) == EINVAL  # an empty formula
        draw = lambda rules, bags='bags', ok='ok': _lib.lib().mg_episode_draw_formulas(E, Z, zs_c, rules, ptr(bags) if bags else None,
                                                                                       ptr(ok) if ok else None, _stream())
        assert draw(edited(sampled, max_tries=0)) == EINVAL and draw(edited(sampled, max_tries=65)) == EINVAL
        assert draw(edited({})) == EINVAL and draw(None) == EINVAL  # rules without sampled formulas
        assert draw(edited(sampled), bags=None) == EINVAL and draw(edited(sampled), ok=None) == EINVAL
        # and the unedited rules are accepted
        assert step(edited({})) == 0 and step(edited(hull)) == 0 and step(edited(sampled)) == 0 and draw(edited(sampled)) == 0
        torch.cuda.synchronize()
