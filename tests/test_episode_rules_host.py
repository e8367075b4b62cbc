"""The host statement of the episode rules (tests/episode_ref.py), pinned to the reference environment's own known answers
(its tests/test_environment.py, given here as literal data), plus the formula cycle and the episode reconstruction.  No GPU."""
import numpy as np
import pytest

from tests import episode_ref as R

ZS = [0, 1, 6, 7, 8]
H2CO = (0, 2, 1, 0, 1)  # bag counts over ZS


def test_addition_h_on_the_empty_canvas_is_placed():
    env = R.RulesEnv(5, ZS, [H2CO])
    obs, reward, done, info = env.step((1, (0.0, 1.0, 0.0)))
    assert obs[0][0] == (1, (0.0, 1.0, 0.0)) and ZS[obs[0][0][0]] == 1
    assert obs[1] == (0, 1, 1, 0, 1)
    assert reward == 0.0 and not done and info['status'] == R.PLACED


def test_solo_distance_second_h_is_done():
    env = R.RulesEnv(5, ZS, [H2CO], max_solo_distance=1.0)
    _, _, done, _ = env.step((1, (0.0, 0.0, 0.0)))  # the first H can be on its own
    assert not done
    obs, reward, done, info = env.step((1, (0.0, 1.5, 0.0)))  # the second cannot: the canvas holds only H
    assert done and info['status'] == R.SOLO and reward == 0.0
    assert obs[1] == (0, 1, 1, 0, 1) and sum(1 for label, _ in obs[0] if label != 0) == 1  # nothing placed


def test_an_element_absent_from_the_bag_is_an_error():
    env = R.RulesEnv(5, ZS, [H2CO])
    with pytest.raises(RuntimeError):
        env.step((3, (0.0, 1.0, 0.0)))  # N
    assert R.decide(ZS, 5, [], np.zeros((0, 3)), H2CO, 3, np.zeros(3), 0.6, 2.0) == R.ERROR
    assert R.decide(ZS, 5, [], np.zeros((0, 3)), H2CO, 5, np.zeros(3), 0.6, 2.0) == R.ERROR  # index out of range
    assert R.decide(ZS, 5, [], np.zeros((0, 3)), H2CO, 0, np.zeros(3), 0.6, 2.0) == R.STOP  # the null element is not in any bag


def test_rule_order_and_thresholds():
    pos = np.array([[0.0, 0.0, 0.0]])
    d = lambda z_new, q, charges=(6, ), p=pos, bag=H2CO, N=5: R.decide(ZS, N, list(charges), p, bag, ZS.index(z_new),
                                                                   np.array(q, dtype=np.float64), 0.5, 2.0)
    assert d(8, (0.5, 0.0, 0.0)) == R.PLACED  # exactly at min_atomic_distance: not too close
    assert d(8, (np.nextafter(0.5, 0.0), 0.0, 0.0)) == R.TOO_CLOSE
    assert d(1, (2.0, 0.0, 0.0)) == R.SOLO  # exactly at max_solo_distance: not covered
    assert d(1, (np.nextafter(2.0, 0.0), 0.0, 0.0)) == R.PLACED
    assert d(1, (0.25, 0.0, 0.0), charges=(1, )) == R.TOO_CLOSE  # too close comes before solo
    assert d(8, (9.0, 0.0, 0.0)) == R.PLACED  # only H, F, Cl, Br need a neighbour
    assert d(8, (1.0, 0.0, 0.0), N=2, bag=(0, 0, 0, 0, 1)) == R.FULL  # full before bag-empty
    assert d(8, (1.0, 0.0, 0.0), bag=(0, 0, 0, 0, 1)) == R.BAG_EMPTY


def _state(E, N, Z, formulas, start=None):
    st = dict(pos64=np.zeros((E, N, 3)), pos32=np.zeros((E, N, 3), dtype=np.float32), charges=np.zeros((E, N), dtype=np.int32),
              bags=np.tile(np.asarray(formulas[0], dtype=np.float32), (E, 1)), natoms=np.zeros(E, dtype=np.int32),
              alive=np.ones(E, dtype=np.int32), episode_no=np.zeros(E, dtype=np.int32),
              formulas=np.asarray(formulas, dtype=np.float32))
    st.update(start_pos64=st['pos64'].copy(), start_charges=st['charges'].copy(), start_natoms=st['natoms'].copy())
    return st


def test_formula_cycle_over_three_formulas():
    formulas = [(0, 2, 0, 0, 1), (0, 4, 1, 0, 0), (0, 0, 1, 0, 2)]
    st = _state(2, 5, 5, formulas)
    stop = np.zeros((2, 7), dtype=np.float32)  # element 0: the null symbol
    newpos = np.zeros((2, 3))
    seen = []
    for k in range(7):
        seen.append(tuple(st['bags'][0]))
        status, element = R.episode_step(st, ZS, stop, newpos, 0.6, 2.0, False)
        assert list(status) == [R.STOP, R.STOP] and list(element) == [0, 0]
        assert list(st['episode_no']) == [k + 1, k + 1]
    assert seen == [tuple(float(c) for c in formulas[k % 3]) for k in range(7)]
    env = R.RulesEnv(5, ZS, formulas)  # the test double cycles the same way
    for k in range(7):
        assert tuple(env.bag) == formulas[k % 3]
        env.step((0, (0.0, 0.0, 0.0)))
        env.reset()


def test_array_model_follows_the_environment_double():
    """the array form (what the kernel is compared with) and RulesEnv take the same decisions on the same actions"""
    rng = np.random.default_rng(3)
    formulas = [(0, 2, 0, 0, 1), (0, 4, 1, 0, 0)]
    E, N = 6, 4
    st = _state(E, N, 5, formulas)
    envs = [R.RulesEnv(N, ZS, formulas, 1.0, 2.0) for _ in range(E)]
    counts = np.zeros(8, dtype=int)
    for _ in range(30):
        acts = np.zeros((E, 7), dtype=np.float32)
        newpos = rng.uniform(-1.5, 1.5, size=(E, 3))
        for e in range(E):
            have = [i for i, c in enumerate(envs[e].bag) if c > 0]
            acts[e, 2] = rng.choice(have + [0])
        status, element = R.episode_step(st, ZS, acts, newpos, 1.0, 2.0, False)
        for e in range(E):
            _, _, done, info = envs[e].step((int(element[e]), tuple(newpos[e])))
            assert info['status'] == status[e]
            if done:
                envs[e].reset()
            canvas, bag = envs[e]._obs()
            assert tuple(st['bags'][e]) == tuple(float(c) for c in bag)
            n = int(st['natoms'][e])
            assert [ZS[label] for label, _ in canvas[:n]] == list(st['charges'][e, :n]) and all(label == 0 for label, _ in canvas[n:])
            assert np.array_equal(np.array([p for _, p in canvas]), st['pos64'][e])
        counts += np.bincount(status, minlength=8)
    assert counts[R.PLACED] and counts[R.TOO_CLOSE] and counts[R.SOLO] and counts[R.STOP] and (counts[R.FULL] or counts[R.BAG_EMPTY])


def test_episode_reconstruction():
    zs = [0, 1, 8]
    f32 = lambda *x: np.array(x, dtype=np.float32)
    P = lambda *rows: np.array(rows, dtype=np.float64)
    records = [
        dict(status=[R.PLACED, R.STOP], element=[2, 0], newpos=P((0, 0, 0), (9, 9, 9)), logp=f32(-1, -2), v=f32(.1, .2)),
        dict(status=[R.PLACED, R.PLACED], element=[1, 2], newpos=P((1, 0, 0), (0, 0, 0)), logp=f32(-3, -4), v=f32(.3, .4)),
        dict(status=[R.BAG_EMPTY, R.TOO_CLOSE], element=[1, 1], newpos=P((0, 1, 0), (.1, 0, 0)), logp=f32(-5, -6), v=f32(.5, .6)),
        dict(status=[R.INACTIVE, R.PLACED], element=[-1, 2], newpos=P((7, 7, 7), (0, 0, 0)), logp=f32(-7, -8), v=f32(.7, .8)),
    ]
    start = ([], [8])
    start_pos = (np.zeros((0, 3)), P((5, 5, 5)))
    eps = R.collect_episodes(records, zs, 2, start, start_pos)
    assert [(e['env'], e['formula'], e['status']) for e in eps] == [(1, 0, R.STOP), (0, 0, R.BAG_EMPTY), (1, 1, R.TOO_CLOSE)]
    assert list(eps[0]['numbers']) == [8] and np.array_equal(eps[0]['positions'], P((5, 5, 5)))  # only the start structure
    assert list(eps[1]['numbers']) == [8, 1, 1] and np.array_equal(eps[1]['positions'], P((0, 0, 0), (1, 0, 0), (0, 1, 0)))
    assert np.array_equal(eps[1]['logp'], f32(-1, -3, -5)) and np.array_equal(eps[1]['v'], f32(.1, .3, .5))
    assert list(eps[2]['numbers']) == [8, 8] and np.array_equal(eps[2]['positions'], P((5, 5, 5), (0, 0, 0)))  # rejected atom left out
    assert np.array_equal(eps[2]['logp'], f32(-4, -6))
    assert R.molecule_obeys_rules(zs, 4, eps[1]['numbers'], eps[1]['positions'], (0, 2, 1), 0, 0.6, 2.0)
    assert not R.molecule_obeys_rules(zs, 4, eps[1]['numbers'], eps[1]['positions'], (0, 2, 1), 0, 1.2, 2.0)  # H-O at 1.0
    assert not R.molecule_obeys_rules(zs, 4, eps[1]['numbers'], eps[1]['positions'], (0, 1, 1), 0, 0.6, 2.0)  # one H too many


def test_the_package_states_the_same_codes_and_bags():
    from molgym_amd import _lib
    from molgym_amd.episodes import formula_to_bag
    assert (_lib.EP_INACTIVE, _lib.EP_PLACED, _lib.EP_STOP, _lib.EP_TOO_CLOSE, _lib.EP_SOLO, _lib.EP_FULL, _lib.EP_BAG_EMPTY,
            _lib.EP_ERROR) == (R.INACTIVE, R.PLACED, R.STOP, R.TOO_CLOSE, R.SOLO, R.FULL, R.BAG_EMPTY, R.ERROR)
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'molgym_hip.h')).read()
    for name in ('INACTIVE', 'PLACED', 'STOP', 'TOO_CLOSE', 'SOLO', 'FULL', 'BAG_EMPTY', 'ERROR'):
        assert int(re.search(rf'#define\s+MG_EP_{name}\s+(\d+)', header).group(1)) == getattr(R, name)
    assert formula_to_bag(((1, 2), (6, 1), (8, 1)), ZS) == H2CO  # string_to_formula('H2CO')
    with pytest.raises(ValueError):
        formula_to_bag(((2, 2), ), ZS)  # He2: the reference's test_invalid_formula
