"""tests/ppo_loss_ref.py without a GPU: the steering reaches every class on any float32 `out`, and the float64 reference takes the
branch each class is named after -- the construction the device tests rest on."""
import numpy as np
import pytest

from tests.ppo_loss_ref import CLASSES, classes_present, classify, reference, steer, steer_zero

CLIP, VF, ENT = 0.2, 0.5, 0.01


def _out(B, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.normal(-5.0, 2.0, B), rng.uniform(0.0, 4.0, B), rng.normal(0.0, 1.0, B)]).astype(np.float32)


@pytest.mark.parametrize('B', [15, 257, 1000])
def test_steer_reaches_every_class_and_the_reference_takes_its_branch(B):
    out = _out(B, seed=B)
    old, adv, ret, labels = steer(out, B, CLIP, seed=1)
    counts = classes_present(labels, need=B // 15)
    assert sum(counts.values()) == B and len(counts) == 15
    assert (classify(out, old, adv, CLIP) == labels).all()
    ref = reference(out, old, adv, ret, CLIP, VF, ENT)
    ratio_class = np.array([s.split('x')[0] for s in labels])
    adv_class = np.array([s.split('x')[1] for s in labels])
    # the clip fraction is the share of the rows labelled above / below / far, exactly
    outside = np.isin(ratio_class, ('above', 'below', 'far'))
    assert (ref['clipped'] == outside).all()
    assert ref['stats'][5] == outside.sum() / B
    g = ref['grad64']
    # ratio exactly 1: min(obj, cobj) ties and the gradient is all of -adv / B
    one = ratio_class == 'one'
    assert (old[one] == out[0].astype(np.float64)[one]).all()
    # (exactly, in the form the mean's adjoint and ppo.inc both take it: the rounded 1 / B times adv.  The single division
    # -adv / B rounds once less and differs from it in the last float64 bit on one row in ten; the float32 coefficients agree.)
    assert (g[0][one] == adv[one] * (-1.0 / B)).all()
    assert (ref['gout'][0][one] == (-adv[one] / B).astype(np.float32)).all()
    assert (g[0][one & (adv_class != 'zero')] != 0.0).all()
    # inside the clip the gradient is that of the unclipped objective
    inside = ratio_class == 'inside'
    ratio = np.exp(out[0].astype(np.float64) - old)
    np.testing.assert_allclose(g[0][inside], (-ratio * adv / B)[inside], rtol=1e-15, atol=0.0)
    # the clipped side passes nothing: above x pos, below x neg, and the far rows on those sides
    delta = out[0].astype(np.float64) - old
    dead = outside & (((delta > 0) & (adv_class == 'pos')) | ((delta < 0) & (adv_class == 'neg')))
    assert dead[(ratio_class == 'above') & (adv_class == 'pos')].all() and dead[(ratio_class == 'below') & (adv_class == 'neg')].all()
    assert (g[0][dead] == 0.0).all()
    far = ratio_class == 'far'
    if B > 15:   # (the second cycle of 15 rows holds the far rows on their clipped side)
        assert (dead & far & (adv_class == 'pos')).any() and (dead & far & (adv_class == 'neg')).any()
    live = outside & ~dead & (adv_class != 'zero')
    assert (live & far).any() and (g[0][live] != 0.0).all() and np.isfinite(g).all()
    assert (g[0][adv_class == 'zero'] == 0.0).all()
    # float32 holds the far rows after the 1 / B
    assert np.isfinite(ref['gout']).all() and (ref['gout'][0][live] != 0.0).all()
    # dv = 0 on every fifth row, and only there
    fifth = np.arange(B) % 5 == 0
    assert (g[2][fifth] == 0.0).all() and (g[2][~fifth] != 0.0).all()
    # the entropy row is one constant
    assert (g[1] == g[1][0]).all() and abs(g[1][0] + ENT / B) <= 1e-16 * ENT / B * 4
    assert abs(ref['ent_mean'] - out[1].astype(np.float64).mean()) == 0.0


def test_gout_rounding_order_and_scale():
    B = 15
    out = _out(B, seed=3)
    old, adv, ret, _ = steer(out, B, CLIP, seed=2)
    r1, r3 = reference(out, old, adv, ret, CLIP, VF, ENT), reference(out, old, adv, ret, CLIP, VF, ENT, gscale=1.0 / 3.0)
    assert r1['gout'].dtype == np.float32 and (r1['gout'] == r1['grad64'].astype(np.float32)).all()
    assert (r3['gout'] == r1['gout'] * np.float32(1.0 / 3.0)).all()
    assert (r3['stats'] == r1['stats']).all()


def test_single_row_is_class_one():
    out = _out(1, seed=4)
    old, adv, ret, labels = steer(out, 1, CLIP, seed=3)
    assert labels.tolist() == ['onexpos'] and old[0] == float(out[0, 0]) and ret[0] == float(out[2, 0])
    ref = reference(out, old, adv, ret, CLIP, VF, ENT)
    assert ref['stats'][5] == 0.0 and ref['stats'][4] == 0.0 and ref['stats'][2] == 0.0
    assert ref['grad64'][0, 0] == -adv[0] and ref['grad64'][2, 0] == 0.0


def test_zero_gradient_batch():
    B = 15
    out = _out(B, seed=5)
    old, adv, ret, labels = steer_zero(out, B, CLIP, seed=4)
    assert set(labels) == {'abovexpos', 'belowxneg'}
    ref = reference(out, old, adv, ret, CLIP, 0.0, 0.0)
    assert (ref['grad64'] == 0.0).all() and (ref['gout'] == 0.0).all() and ref['stats'][5] == 1.0


def test_classes_present_refuses_a_missing_class_and_a_stray_row():
    out = _out(30, seed=6)
    old, adv, ret, labels = steer(out, 30, CLIP, seed=5)
    with pytest.raises(AssertionError):
        classes_present(labels, need=3)
    with pytest.raises(AssertionError):
        classes_present(labels[:14])
    bumped = out.copy()
    bumped[0, 0] = np.nextafter(bumped[0, 0], np.float32(0.0))   # a log-probability one float32 ulp off the one steered from
    stray = classify(bumped, old, adv, CLIP)
    assert stray[0] == '?' and set(stray[1:]) <= set(CLASSES)
    with pytest.raises(AssertionError):
        classes_present(stray)
