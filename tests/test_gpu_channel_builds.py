"""Odd channel-count builds of the library held to the float64 oracle on every launch path.

`num_channels_hidden` (CH) and `num_channels_per_element` (CE) are compile-time constants of a library build.  Odd values take
code no even build reaches: the scalar `else` branches of the edge-level and level-0 kernels (2 CH and EL_K = 2 CH 7 no multiple of
4) and the guarded / unaligned forms behind the host's alignment gates (R = 2 CH, K = 2 CH (2 nblk + 1), R0 = 2 Z CE).

Builds (all at num_cg_levels = 3, prebuilt by __graft_entry__.build()):
  (7, 3)  odd in both counts; R0 = 18 / 30 at Z = 3 / 5
  (9, 5)  the largest odd CH with the maximum CE; R0 = 30 / 50, 2 NLM CE = 250 of the 256 threads
  (1, 1)  the degenerate end: 2 CH = 2, EL_K = 14, R0 = 6 (below the column forms' minimum of 8)
  (8, 2)  even; the only prebuilt build that reaches k_gemm_mfma_sx<1> (2 CH <= 16) at its natural size (boundary case only)

Shapes (the smallest that reach their launch path):
  S    cfg2 (canvas 7, Z = 3), make_batch(12): the fused per-level kernels
  G    cfg4 (canvas 20, Z = 5), crowded canvases [20, 17, 19]: neighbour tiles, the two-kernel list build, the staged edge levels
  e41  cfg4, 41 full canvases: 16 400 edges, above the 16 384 from which even builds keep the DotMatrix block once (shared layout);
       odd builds keep the plain layout at every size (state.inc::ws_build)

Bounds are the project's own (tests/helpers.py): outputs rel_err < 1e-5, gradients assert_grads (2e-4 of the slot maximum, 1e-2
relative on the entries above 1 % of it)."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from molgym_amd.synthetic import make_batch
from tests.helpers import (PPO_HP as HP, ZERO_SLOT, assert_grads, crowded as _crowded, device_batch as _batch, encoder_stage_report, grad_report,
                           make_pair, n_terms as _n_terms, oracle_backward, rel_err, report_vs_float32 as _report_vs_float32)

pytestmark = pytest.mark.gpu
ODD_BUILDS = [(7, 3), (9, 5), (1, 1)]


def _pair(build, shape):
    ch, ce = build
    return make_pair('cfg2' if shape == 'S' else 'cfg4', seed=100 + 10 * ch + ce, num_channels_hidden=ch, num_channels_per_element=ce)


def _data(shape):
    if shape == 'S':
        return make_batch(12, 7, [0, 9, 16], seed=33)
    if shape == 'G':
        return _crowded('cfg4', [20, 17, 19], 7)
    raise KeyError(shape)


def _ids(v):
    return 'c%de%d' % v if isinstance(v, tuple) else str(v)


# ---- parity: outputs and every parameter gradient against the oracle ----------------------------------------------------------
@pytest.mark.parametrize('shape', ['S', 'G'])
@pytest.mark.parametrize('build', ODD_BUILDS, ids=_ids)
def test_channel_builds_small_vs_oracle(built_lib, build, shape):
    from molgym_amd import _lib, layout
    ac, ref, cfg = _pair(build, shape)
    lib = ac._L()
    got = [C.c_int32() for _ in range(4)]
    lib.mg_cov_build_params(*[C.byref(g) for g in got])
    assert [g.value for g in got] == [build[0], build[1], 4, 3] and lib is not _lib.lib()
    n = C.c_int64()
    _lib.check(lib.mg_cov_num_params(C.byref(ac._make_cfg(1, np.array([1]))), C.byref(n)), lib)
    table, total = layout.offsets(len(cfg['zs']), 128, 3, build[0], build[1])
    assert n.value == total == ac.theta.numel() == sum(p.numel() for p in ref.parameters())
    data = _data(shape)
    B = len(data['obs'])
    g = torch.Generator().manual_seed(2)
    wl, we, wv = (torch.randn(B, generator=g, dtype=torch.float64) * s for s in (1.0, 0.3, 0.7))
    out = ac.step(data['obs'], data['act'])
    (out['logp'].double() * wl.cuda() + out['ent'].double() * we.cuda() + out['v'].double() * wv.cuda()).sum().backward()
    torch.cuda.synchronize()
    exp, want = oracle_backward(ref, data, (wl, we, wv))
    # assert_grads passes a slot below 1e-10 over as empty: only the focus head's output bias (zero in exact arithmetic) may be one
    empty = [k for k in ac.slot_table if not want[k].grad.abs().max().item() >= 1e-10]
    assert set(empty) <= {ZERO_SLOT}, empty
    errs = {k: rel_err(out[k].detach(), exp[k].detach()) for k in ('logp', 'ent', 'v')}
    report = grad_report(ac.theta.grad.detach().double().cpu(), want, ac.slot_table)
    worst = max(((v[0], k) for k, v in report.items() if v[1] >= 1e-10))
    print(f'\nbuild {build} shape {shape}: outputs {errs}; worst gradient slot (err / slot max) {worst[0]:.3e} {worst[1]}')
    assert all(bool(torch.isfinite(out[k]).all()) for k in errs) and bool(torch.isfinite(ac.theta.grad).all())
    for k, e in errs.items():
        assert e < 1e-5, (k, e)
    assert_grads(report)


# ---- localisation: every saved encoder intermediate -----------------------------------------------------------------------------
@pytest.mark.parametrize('shape', ['S', 'G'])
def test_channel_builds_encoder_stages(built_lib, shape):
    ac, ref, cfg = _pair((7, 3), shape)
    report = encoder_stage_report(ac, ref, cfg, _data(shape))
    assert len(report) == 3 + 15 + 5 + 1
    bad = {k: v for k, v in report.items() if not v < 1e-5}
    assert not bad, f'stages off: {bad}; all: {report}'


# ---- the one-call PPO step against the autograd path ----------------------------------------------------------------------------
@pytest.mark.parametrize('build', [(7, 3), (9, 5)], ids=_ids)
def test_channel_builds_one_call_step_vs_autograd(built_lib, build):
    from molgym_amd import ppo as ppo_mod
    ac, _, _ = _pair(build, 'S')
    data = _data('S')
    ac.theta.grad = None
    loss, info = ppo_mod.compute_loss(ac, data, *HP)
    loss.backward()
    torch.cuda.synchronize()
    g_auto = ac.theta.grad.detach().clone()
    assert torch.isfinite(g_auto).all() and g_auto.abs().max().item() > 0
    batch = _batch(ac, data)
    for epoch_cache in (False, True):
        ac.theta.grad = torch.zeros_like(ac.theta)
        ac.invalidate_weights()
        stats = ac.ppo_minibatch(batch, *HP, loss_scale=0.5, epoch_cache=epoch_cache).clone()
        ac.ppo_minibatch(batch, *HP, loss_scale=0.5, epoch_cache=epoch_cache)
        ac.fold_gradients()
        torch.cuda.synchronize()
        err = (ac.theta.grad - g_auto).abs().max().item()
        print(f'\nbuild {build} epoch_cache {epoch_cache}: |step - autograd| {err:.3e} of {g_auto.abs().max().item():.3e}')
        assert err <= 2e-5 * max(1.0, g_auto.abs().max().item()), epoch_cache
        assert abs(stats[3].item() - info['total_loss']) <= 1e-6 * max(1.0, abs(info['total_loss']))


# ---- rollout: what the sampling launch reports for its draws is what evaluation gives -------------------------------------------
@pytest.mark.parametrize('build', [(7, 3), (1, 1)], ids=_ids)
def test_channel_builds_rollout_draws_evaluate_the_same(built_lib, build):
    ac, _, _ = _pair(build, 'S')
    data = _data('S')
    ac.training = True
    torch.manual_seed(0)
    drawn = ac.step(data['obs'])
    again = ac.step(data['obs'], drawn['a'].cpu().numpy())
    assert torch.isfinite(drawn['logp']).all() and torch.isfinite(drawn['v']).all()
    assert (drawn['logp'] - again['logp']).abs().max().item() < 1e-4 and (drawn['v'] - again['v']).abs().max().item() < 1e-5


# ---- the 16 384-edge layout boundary under default switches ---------------------------------------------------------------------
def _take(data, ix):
    return {'obs': [data['obs'][i] for i in ix], **{k: np.asarray(data[k])[ix] for k in ('act', 'logp', 'adv', 'ret')}}


@pytest.mark.parametrize('build', [(7, 3), (8, 2)], ids=_ids)
def test_channel_builds_across_the_layout_boundary(built_lib, build):
    """41 full canvases of 20 = 16 400 edges in ONE step, against the two halves (8 000 and 8 400 edges: the plain layout, which the
    parity case holds to the oracle) taken alone.  The PPO loss is a mean over the samples, so the gradient of the whole is the
    sum of the halves' gradients at loss_scale 20/41 and 21/41.  Outputs of the first two and last two canvases against the
    float64 oracle on those four alone (samples are independent).
    What is independent here: the step not raising, and the four outputs against the oracle.  For (7, 3) the whole and the halves
    both run the plain layout through the same kernels (at other grid sizes, and the whole with the side stream of >= 16 384
    edges), so its gradient comparison is a self-consistency check; for (8, 2) the whole runs the shared layout (k_gemm_mfma_sx<1>,
    k_gemm_mfma_pk) against halves on the plain one, which the oracle holds in tests/test_gpu_parity_full.py."""
    ac, ref, _ = make_pair('cfg4', seed=51, num_channels_hidden=build[0], num_channels_per_element=build[1])
    data = _crowded('cfg4', [20] * 41, 52)
    assert sum(len([1 for it in o[0] if it[0] != 0]) ** 2 for o in data['obs']) == 16400
    other = copy.deepcopy(ac)
    other.theta.grad = torch.zeros_like(other.theta)
    for ix in (list(range(20)), list(range(20, 41))):
        other.ppo_minibatch(_batch(other, _take(data, ix)), *HP, loss_scale=len(ix) / 41.0)
    torch.cuda.synchronize()
    g_halves = other.theta.grad.clone()
    ac.theta.grad = torch.zeros_like(ac.theta)
    stats = ac.ppo_minibatch(_batch(ac, data), *HP).clone()   # (must not raise)
    torch.cuda.synchronize()
    out = ac._last_out.clone()
    g_whole = ac.theta.grad.clone()
    assert torch.isfinite(stats).all() and torch.isfinite(g_whole).all() and torch.isfinite(g_halves).all()
    assert g_halves.abs().max().item() > 0
    report = _report_vs_float32(g_whole, g_halves, ac.slot_table, _n_terms(data))
    print(f'\nbuild {build}: worst gradient slot, 41 canvases against the halves (err / slot max):',
          max(v[0] for v in report.values() if v[1] >= 1e-10))
    assert_grads(report)
    ix = [0, 1, 39, 40]
    four = _take(data, ix)
    with torch.no_grad():
        exp = ref.step(four['obs'], four['act'], dtype=torch.float64)
    for row, k in enumerate(('logp', 'ent', 'v')):
        err = rel_err(out[row][ix], exp[k])
        print(k, err)
        assert err < 1e-5, (k, err)
