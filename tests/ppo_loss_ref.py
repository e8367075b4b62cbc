"""Steered PPO batches and the float64 reference of the loss (tests/test_ppo_loss_ref_host.py pins this file on the CPU;
tests/test_gpu_ppo_loss_classes.py holds every copy of the loss on the device to it).

The step tests draw `logp` from N(-5, 1): the ratio is arbitrary and nearly every row is clipped.  Here the old log-probabilities
are built FROM the float32 outputs the kernel itself returned, so that every row sits in a branch chosen beforehand:

  ratio classes (delta = logp - old_logp)      advantage classes
    one      old_logp = float64(out[0, b])       pos    uniform in [0.1, 2]
    inside   |delta| in [0.01, 0.1], both signs  neg    uniform in [-2, -0.1]
    above    delta in [0.3, 2]                   zero   exactly 0.0
    below    delta in [-2, -0.3]
    far      delta = +-40

Row b takes combination b % 15 (ratio class (b % 15) // 3, advantage class b % 3): B = 15 holds each once, B = 1 holds
`one` x `pos`.  Every fifth row has ret = float64(out[2, b]): dv = 0 exactly.  No row sits within 5 % of a clip boundary (asserted
for the clip ratio given), so float32 and float64 never disagree about a branch.  A `far` row starts on the side on which the
objective is NOT clipped (-40 with a positive advantage: a ratio of 4e-18; +40 with a negative one: 2e17, finite in float32 after
the 1 / B) and changes side with every cycle of 15 rows."""
import numpy as np
import torch

from oracle.ppo_ref import loss_from_pred

RATIO_CLASSES = ('one', 'inside', 'above', 'below', 'far')
ADV_CLASSES = ('pos', 'neg', 'zero')
CLASSES = tuple(f'{r}x{a}' for r in RATIO_CLASSES for a in ADV_CLASSES)
FAR = 40.0
GOUT_RTOL = 2.5e-7   # two float32 roundings of 2^-24 each (the gradient, the scale) + a device exp within an ulp of float64
STAT_RTOL = 1e-12    # the suite's bound for these float64 sums (tests/test_gpu_ppo.py)


def _out64(out):
    out = out.detach().cpu().numpy() if torch.is_tensor(out) else np.asarray(out)
    assert out.dtype == np.float32 and out.ndim == 2 and out.shape[0] == 3, (out.dtype, out.shape)
    return out.astype(np.float64)


def _check_margins(clip):
    lo, hi = 1.0 - clip, 1.0 + clip
    assert np.exp(0.1) < 0.95 * hi and np.exp(-0.1) > 1.05 * lo, clip     # `inside` stays 5 % inside the boundaries
    assert np.exp(0.3) > 1.05 * hi and np.exp(-0.3) < 0.95 * lo, clip     # `above` / `below` 5 % outside them


def classify(out, old_logp, adv, clip):
    """the class label of every row, from the outputs a step RETURNED and the batch it ran on; '?' for a row in no class (a
    forward that is not the one the batch was steered from: classes_present then fails)"""
    _check_margins(clip)
    o = _out64(out)
    delta = o[0] - np.asarray(old_logp, dtype=np.float64)
    adv = np.asarray(adv, dtype=np.float64)
    labels = []
    for d, a in zip(delta, adv):
        m = abs(d)
        # (delta is a difference of two float64 numbers near |logp| <~ 100: a steered 0.01 comes back to 1e-14)
        r = 'one' if d == 0.0 else 'inside' if 0.01 - 1e-9 <= m <= 0.1 + 1e-9 else 'above' if 0.3 - 1e-9 <= d <= 2.0 + 1e-9 else \
            'below' if -2.0 - 1e-9 <= d <= -0.3 + 1e-9 else 'far' if abs(m - FAR) <= 1e-9 else '?'
        s = 'pos' if a > 0.0 else 'neg' if a < 0.0 else 'zero'
        labels.append('?' if r == '?' else f'{r}x{s}')
    return np.array(labels)


def steer(out, B, clip, seed):
    """old_logp, adv, ret (float64 numpy) and the class label per row for the kernel's own float32 `out` ([3, B]: logp, ent, v)"""
    _check_margins(clip)
    o = _out64(out)
    assert o.shape[1] == B and np.isfinite(o).all()
    rng = np.random.default_rng(seed)
    b = np.arange(B)
    rc, ac, cycle = (b % 15) // 3, b % 3, b // 15
    sign = np.where(rng.random(B) < 0.5, -1.0, 1.0)
    mag = {1: rng.uniform(0.01, 0.1, B), 2: rng.uniform(0.3, 2.0, B), 3: rng.uniform(0.3, 2.0, B)}
    # far: the unclipped side first (delta < 0 for a positive advantage, > 0 otherwise), the other side in every second cycle
    far_sign = np.where(ac == 0, -1.0, 1.0) * np.where(cycle % 2 == 0, 1.0, -1.0)
    delta = np.select([rc == 0, rc == 1, rc == 2, rc == 3], [np.zeros(B), sign * mag[1], mag[2], -mag[3]], FAR * far_sign)
    old_logp = np.where(rc == 0, o[0], o[0] - delta)
    amp = rng.uniform(0.1, 2.0, B)
    adv = np.select([ac == 0, ac == 1], [amp, -amp], 0.0)
    ret = np.where(b % 5 == 0, o[2], rng.normal(0.0, 1.0, B))
    labels = classify(out, old_logp, adv, clip)
    want = np.array([f'{RATIO_CLASSES[r]}x{ADV_CLASSES[a]}' for r, a in zip(rc, ac)])
    assert (labels == want).all(), (labels[labels != want], want[labels != want])
    return old_logp, adv, ret, labels


def steer_zero(out, B, clip, seed):
    """a batch whose every row is `above` x `pos` or `below` x `neg`: the clipped side of both, d loss / d logp = 0 in every row"""
    _check_margins(clip)
    o = _out64(out)
    assert o.shape[1] == B
    rng = np.random.default_rng(seed)
    up = np.arange(B) % 2 == 0
    mag, amp = rng.uniform(0.3, 2.0, B), rng.uniform(0.1, 2.0, B)
    old_logp, adv = o[0] - np.where(up, mag, -mag), np.where(up, amp, -amp)
    labels = classify(out, old_logp, adv, clip)
    assert set(labels) <= {'abovexpos', 'belowxneg'}
    return old_logp, adv, rng.normal(0.0, 1.0, B), labels


def classes_present(labels, need=1, classes=CLASSES):
    """every class holds at least `need` rows and no row is outside the classes; asserted BEFORE anything is compared"""
    labels = np.asarray(labels)
    counts = {c: int((labels == c).sum()) for c in classes}
    assert not (labels == '?').any(), ('rows in no class', np.nonzero(labels == '?')[0].tolist())
    short = {c: n for c, n in counts.items() if n < need}
    assert not short, (f'classes with fewer than {need} rows', short)
    return counts


def reference(out, old_logp, adv, ret, clip, vf, ent, gscale=1.0):
    """oracle.ppo_ref.loss_from_pred on float64 leaf copies of `out`, differentiated by autograd ->
      stats     the six statistics (float64; the clip fraction as count / B, the reference's own is a float32 mean)
      ent_mean  mean of out[1] in float64
      clipped   the rows the reference counts as clipped (bool)
      grad64    d loss / d (logp, ent, v), [3, B] float64
      gout      float32(float32(grad64) * float32(gscale)): the rounding order ppo.inc documents
      summand   per statistic, the largest |term| of its sum (the tolerance of a sum that cancels is absolute in it)"""
    o = _out64(out)
    B = o.shape[1]
    logp, e, v = (torch.tensor(o[k], dtype=torch.float64, requires_grad=True) for k in range(3))
    old, a, r = (torch.as_tensor(np.asarray(x, dtype=np.float64)) for x in (old_logp, adv, ret))
    loss, info = loss_from_pred(logp, e, v, old, a, r, clip, vf, ent)
    loss.backward()
    grad64 = np.stack([logp.grad.numpy(), e.grad.numpy(), v.grad.numpy()])
    with torch.no_grad():
        ratio = torch.exp(logp - old)
        clipped = (ratio.lt(1 - clip) | ratio.gt(1 + clip)).numpy()
        terms = [torch.min(ratio * a, ratio.clamp(1 - clip, 1 + clip) * a).abs().max().item(), abs(ent) * e.abs().max().item(),
                 abs(vf) * (v - r).pow(2).max().item(), 0.0, (old - logp).abs().max().item(), 1.0]
        terms[3] = max(terms[:3])
    stats = np.array([info['policy_loss'], info['entropy_loss'], info['vf_loss'], info['total_loss'], info['approx_kl'],
                      float(clipped.sum()) / B])
    gout = (grad64.astype(np.float32) * np.float32(gscale)).astype(np.float32)
    return dict(stats=stats, ent_mean=float(o[1].mean()), clipped=clipped, grad64=grad64, gout=gout, summand=np.array(terms))


def assert_gout(got, want, tag=''):
    """`got` (the kernel's float32 coefficients) against reference()['gout']: equal where the reference is 0 and on the whole entropy
    row (a constant), relative error <= GOUT_RTOL elsewhere"""
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.dtype == np.float32 and got.shape == want.shape, (tag, got.dtype, got.shape)
    assert np.isfinite(got).all(), tag
    zero = want == 0.0
    assert (got[zero] == 0.0).all(), (tag, 'non-zero where the reference is 0', np.argwhere(zero & (got != 0.0)).tolist()[:8])
    assert (got[1] == want[1]).all(), (tag, 'entropy row', got[1][:4], want[1][:4])
    g, w = got[~zero].astype(np.float64), want[~zero].astype(np.float64)
    rel = np.abs(g - w) / np.abs(w)
    worst = float(rel.max()) if rel.size else 0.0
    print(f'{tag}: gout worst relative error {worst:.3g} over {rel.size} entries, {int(zero.sum())} exact zeros')
    assert worst <= GOUT_RTOL, (tag, worst, np.argwhere(~zero)[int(rel.argmax())].tolist())


def assert_stats(got, ref, tag=''):
    """six float64 statistics against reference(): rtol 1e-12, atol 1e-12 x the largest |summand| of each; the clip fraction within
    1e-15 of count / B"""
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.dtype == np.float64 and got.shape == (6, ), (tag, got.dtype, got.shape)
    want = ref['stats']
    err = np.abs(got - want)
    print(f'{tag}: stats |err| {err.tolist()} of {want.tolist()}')
    assert np.isfinite(got).all(), (tag, got)
    bound = STAT_RTOL * np.abs(want) + 1e-12 * ref['summand']
    assert (err[:5] <= bound[:5]).all(), (tag, err.tolist(), bound.tolist())
    assert err[5] <= 1e-15, (tag, got[5], want[5])
