"""Every copy of the PPO loss against float64, on batches steered into every branch (tests/ppo_loss_ref.py).

The loss is written eight times: ppo_loss_body in k_ppo_loss; ppo_loss_gout_one / _pre in k_heads_fwd, k_int_heads_eval,
k_int_heads_fwd<8|16> and k_int_heads_fwd_pre<8|16>; the statistics riders of their adjoint kernels.  Which copy runs depends on
agent, canvas, width and mode.  The step tests' batches (`make_batch`: logp ~ N(-5, 1)) clip nearly every row; here the old
log-probabilities are built from the outputs the step itself returned, so that the ratio is exactly 1, inside the clip, outside it
on either side and 40 away from it, against positive, negative and zero advantages -- asserted from the returned outputs before
anything is compared.

  A1  mg_ppo_loss alone at B = 1, 15, 255 | 256 | 257 (block_sum_d's seam) and 1000 (the strided loop)
  A2  the loss inside ppo_minibatch on every default launch path that hosts it; the launch log names the kernel that ran.  `gout`
      (the seed of the whole backward) against the reference and, bit for bit, against the stand-alone kernel on the returned
      outputs -- ppo.inc's "same float64 arithmetic, same roundings"; a batch whose every row is clipped on the dead side leaves
      gout and theta.grad exactly zero.

Tolerances (tests/ppo_loss_ref.py: GOUT_RTOL, assert_stats) are derived from the number formats, none from the kernels."""
import ctypes as C

import numpy as np
import pytest
import torch

from molgym_amd import _lib
from molgym_amd.spaces import ActionSpace, ObservationSpace
from molgym_amd.synthetic import make_batch, make_batch_internal
from tests.helpers import PPO_HP, launch_log, make_pair
from tests.ppo_loss_ref import (assert_gout, assert_stats, classes_present, classify, reference, steer, steer_zero)

pytestmark = pytest.mark.gpu
P = lambda t: C.c_void_p(t.data_ptr())
S = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
CLIP, VF, ENT = PPO_HP
THIRD = 1.0 / 3.0   # (not a float32 number: the scale's own rounding is part of the coefficient)


def _standalone(lib, out, old, adv, ret, hp=PPO_HP):
    """mg_ppo_loss on `out` (device float32 [3, B]) -> (stats, gout)"""
    B = out.shape[1]
    dev = lambda x: torch.as_tensor(np.asarray(x, dtype=np.float64)).cuda()
    old, adv, ret = dev(old), dev(adv), dev(ret)
    stats = torch.full((6, ), float('nan'), dtype=torch.float64, device='cuda')
    gout = torch.full((3, B), float('nan'), dtype=torch.float32, device='cuda')
    _lib.check(lib.mg_ppo_loss(B, P(out), P(old), P(adv), P(ret), *hp, P(stats), P(gout), S()))
    torch.cuda.synchronize()
    return stats, gout


# ---- A1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [1, 15, 255, 256, 257, 1000])
def test_ppo_loss_kernel_on_every_class(built_lib, B):
    rng = np.random.default_rng(100 + B)
    out = torch.from_numpy(np.stack([rng.normal(-5.0, 2.0, B), rng.uniform(0.0, 4.0, B),
                                     rng.normal(0.0, 1.0, B)]).astype(np.float32)).cuda()
    old, adv, ret, labels = steer(out, B, CLIP, seed=B)
    if B == 1:
        assert labels.tolist() == ['onexpos']
    else:
        classes_present(labels, need=B // 15)
    stats, gout = _standalone(built_lib, out, old, adv, ret)
    ref = reference(out, old, adv, ret, CLIP, VF, ENT)
    assert_gout(gout, ref['gout'], f'mg_ppo_loss[B={B}]')
    assert_stats(stats, ref, f'mg_ppo_loss[B={B}]')
    # the statistics without coefficients (gout = null) are the same launch's
    only = torch.full((6, ), float('nan'), dtype=torch.float64, device='cuda')
    d_old, d_adv, d_ret = (torch.as_tensor(x).cuda() for x in (old, adv, ret))
    _lib.check(built_lib.mg_ppo_loss(B, P(out), P(d_old), P(d_adv), P(d_ret), CLIP, VF, ENT, P(only), None, S()))
    torch.cuda.synchronize()
    assert torch.equal(only, stats)


# ---- A2 ---------------------------------------------------------------------------------------------------------------------
def _schnet(canvas, width, seed):
    from molgym_amd.agents.internal import SchNetAC
    zs = [0, 9, 16]
    torch.manual_seed(seed)
    ac = SchNetAC(ObservationSpace(canvas, zs), ActionSpace(zs), (0.8, 1.8), width, device='cuda:0')
    with torch.no_grad():
        g = torch.Generator().manual_seed(seed + 1)
        for name, (off, shape) in ac.slot_table.items():
            n = int(np.prod(shape))
            if name.endswith('bias'):
                ac.theta[off:off + n] = (0.1 * torch.randn(n, generator=g)).to(ac.theta)
    return ac, zs


class _switch:
    """a process-wide switch of the library for the block: `setter(1)` returns the previous value, restored on the way out"""

    def __init__(self, setter):
        self.setter = setter

    def __enter__(self):
        self.prev = self.setter(1) if self.setter is not None else None

    def __exit__(self, *exc):
        if self.setter is not None:
            self.setter(self.prev)
        return False


# case -> (agent, width, canvas, B, kernel of the coefficients, kernel of the statistics, kernels that must NOT have run, switch,
#          (graph argument, last_step_used_graph expected) ...)
BOTH = ((False, False), (True, True))
CASES = {
    'cov_fused_b15': ('cov', 128, 7, 15, 'k_heads_fwd', 'k_heads_bwd', ('k_ppo_loss', ), None, BOTH),
    'cov_fused_b257': ('cov', 128, 7, 257, 'k_heads_fwd', 'k_heads_bwd', ('k_ppo_loss', ), None, BOTH),
    # staged heads: the adjoint zeroes its accumulators with a memset, which a recorded step cannot hold -- the library runs
    # the launches on the stream whatever `graph` asks for
    'cov_staged_b15': ('cov', 256, 7, 15, 'k_ppo_loss', 'k_ppo_loss', ('k_heads_fwd', 'k_heads_bwd'), None, ((False, False), (True, False))),
    # the ordered switch gives up the one-launch heads and the graph: the cfg2 shape then takes k_ppo_loss as its own launch
    'cov_ordered_b15': ('cov', 128, 7, 15, 'k_ppo_loss', 'k_ppo_loss', ('k_heads_fwd', 'k_heads_bwd'), 'ordered', ((False, False), )),
    'int_pre8_b15': ('int', 128, 7, 15, 'k_int_heads_fwd_pre<8>', 'k_int_heads_bwd_pre<8>', ('k_ppo_loss', 'k_int_heads_eval'), None, BOTH),
    'int_pre8_b257': ('int', 128, 7, 257, 'k_int_heads_fwd_pre<8>', 'k_int_heads_bwd_pre<8>', ('k_ppo_loss', 'k_int_heads_eval'), None, BOTH),
    'int_pre16_b15': ('int', 128, 12, 15, 'k_int_heads_fwd_pre<16>', 'k_int_heads_bwd_pre<16>', ('k_ppo_loss', 'k_int_heads_eval'), None, BOTH),
    'int_grouped_b15': ('int', 128, 20, 15, 'k_int_heads_eval<1>', 'k_int_heads_eval_bwd<1>', ('k_ppo_loss', 'k_int_heads_fwd', 'k_int_heads_fwd_pre'), None, BOTH),
    'int_w64_b15': ('int', 64, 7, 15, 'k_int_heads_fwd<8>', 'k_int_heads_bwd<8>', ('k_ppo_loss', 'k_int_heads_fwd_pre', 'k_int_heads_eval'), None, BOTH),
    'int_deterministic_b15': ('int', 128, 7, 15, 'k_int_heads_fwd_pre<8>', 'k_int_heads_bwd_pre<8>', ('k_ppo_loss', ), 'deterministic', ((False, False), )),
}


def _write(batch, old, adv, ret):
    for dst, src in ((batch.logp, old), (batch.adv, adv), (batch.ret, ret)):
        dst.copy_(torch.from_numpy(np.ascontiguousarray(src)))   # in place: the batch's own device tensors


@pytest.mark.parametrize('case', list(CASES))
def test_loss_inside_the_step(built_lib, case):
    """1. ppo_minibatch once with throw-away gradients for `out`; 2. steer from it; 3. batch.logp / adv / ret written in place;
    4. the step again on a zeroed theta.grad, per (graph, loss_scale); 5. out, gout, stats, stats_accum read and compared."""
    kind, width, canvas, B, k_coef, k_stats, k_not, switch, modes = CASES[case]
    if kind == 'cov':
        ac, _, cfg = make_pair('cfg2', seed=61, network_width=width)
        assert cfg['canvas_size'] == canvas
        data = make_batch(B, canvas, cfg['zs'], seed=62)
        lib = ac._L()
    else:
        ac, zs = _schnet(canvas, width, seed=63)
        data = make_batch_internal(B, canvas, zs, seed=64)
        lib = built_lib
    setter = {None: None, 'ordered': lib.mg_cov_set_ordered, 'deterministic': lib.mg_set_deterministic}[switch]
    batch = ac.prepare_batch(data['obs'], data['act'], data['logp'], data['adv'], data['ret'])
    third32 = torch.tensor(np.float32(THIRD), device='cuda')
    with _switch(setter):
        ac.theta.grad = torch.zeros_like(ac.theta)
        ac.ppo_minibatch(batch, *PPO_HP, graph=False)
        torch.cuda.synchronize()
        out0 = ac._last_out.clone()
        old, adv, ret, _ = steer(out0, B, CLIP, seed=65)
        zero = steer_zero(out0, B, CLIP, seed=66)
        seen = {}
        for graph, expect_graph in modes:
            for scale in (1.0, THIRD):
                tag = f'{case}[graph={graph}, scale={scale:.3g}]'
                _write(batch, old, adv, ret)
                acc = torch.zeros(6, dtype=torch.float64, device='cuda')
                ac.theta.grad.zero_()
                with launch_log(lib) as log:
                    stats = ac.ppo_minibatch(batch, *PPO_HP, loss_scale=scale, stats_accum=acc, graph=graph)
                torch.cuda.synchronize()
                assert ac.last_step_used_graph == expect_graph, (tag, ac.last_step_used_graph)
                out, gout, stats, acc1 = ac._last_out.clone(), ac._last_gout.clone(), stats.clone(), acc.clone()
                assert log.ran(k_coef) and log.ran(k_stats), (tag, sorted(set(log.names)))
                assert not any(log.ran(k) for k in k_not), (tag, sorted(set(log.names)))
                # classes, from the outputs THIS step returned
                classes_present(classify(out, old, adv, CLIP), need=B // 15)
                # against the reference
                ref = reference(out, old, adv, ret, CLIP, VF, ENT, gscale=scale)
                assert_gout(gout, ref['gout'], tag)
                assert_stats(stats, ref, tag)
                # against the stand-alone kernel on the returned outputs: the coefficients bit for bit
                s_stats, s_gout = _standalone(lib, out, old, adv, ret)
                want = s_gout if scale == 1.0 else s_gout * third32
                assert torch.equal(gout, want), (tag, (gout != want).nonzero()[:8].tolist())
                assert_stats(stats, dict(ref, stats=s_stats.cpu().numpy()), tag + ' vs mg_ppo_loss')
                # the same device code on the same outputs: the same bits
                key = (scale, )
                if key in seen and torch.equal(seen[key][0], out):
                    assert torch.equal(seen[key][1], gout), tag
                seen.setdefault(key, (out, gout))
                # the epoch accumulator: loss_scale x statistics, over two calls
                assert torch.allclose(acc1, scale * stats, rtol=1e-14, atol=0), (tag, acc1, stats)
                stats2 = ac.ppo_minibatch(batch, *PPO_HP, loss_scale=scale, stats_accum=acc, graph=graph).clone()
                torch.cuda.synchronize()
                assert torch.allclose(acc, scale * stats + scale * stats2, rtol=1e-14, atol=0), (tag, acc, stats, stats2)
            # every row clipped on its dead side, no value or entropy term: nothing of the backward may turn a zero seed into a
            # number or a NaN
            tag = f'{case}[graph={graph}, zero seed]'
            _write(batch, *zero[:3])
            ac.theta.grad.zero_()
            stats = ac.ppo_minibatch(batch, CLIP, 0.0, 0.0, graph=graph).clone()
            torch.cuda.synchronize()
            assert ac.last_step_used_graph == expect_graph, tag
            out, gout, grad = ac._last_out, ac._last_gout, ac.theta.grad
            assert set(classify(out, zero[0], zero[1], CLIP)) == {'abovexpos', 'belowxneg'}, tag
            assert (gout == 0).all(), (tag, gout.abs().max().item())
            assert torch.isfinite(grad).all() and (grad == 0).all(), (tag, int((grad != 0).sum()), grad.abs().max().item())
            ref = reference(out, *zero[:3], CLIP, 0.0, 0.0)
            assert_stats(stats, ref, tag)
            assert abs(stats[5].item() - 1.0) <= 1e-15 and stats[1].item() == 0.0 and stats[2].item() == 0.0
