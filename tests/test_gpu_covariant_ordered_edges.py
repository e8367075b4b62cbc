"""CovariantAC's ordered mode where a store-to-scratch-then-fold form goes wrong and an atomic-add-into-zeros form cannot: a slot that
is folded but never stored (the three scratch regions poisoned before the step), a region that is too small (guard bands around a
workspace of exactly the reported size; refusals of smaller ones), the instantiations and loop trips the other ordered tests do not
reach, the 16 384-edge boundary of the default mode's shared DotMatrix layout with flips of the switch inside an epoch, and the
other builds and configurations in the mode.

Shapes (the smallest that reach the path):
  a    cfg4, atom counts 0, 1, 8, 9, 16, 17, 20 (case (c) of tests/test_gpu_covariant_deterministic.py)
  b1/2 cfg2 elements on a canvas of 8, counts [8] and [8, 1]: TE = 64 / 65 = one / two workgroups of k_phi_bwd<true>
  c    cfg2 with num_gaussians = 8 (GMM_MAXG), 260 full canvases of 7: TA = 1820 >= 1639 (k_catbuild_bwd_mfma<true, true>), B > 256
       (second trip of k_gmm_logstd_bwd_ord's stride loop), TE = 12 740 (below the layout threshold)
  d    canvas 65, counts 0, 64, 65 (tests/test_gpu_wide_canvas.py::test_covariant_vs_oracle: staged heads, both sides of 64 lanes)
  e40 / e41  cfg4, 40 / 41 full canvases of 20: 16 000 / 16 400 edges, either side of sx_min_rows"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from molgym_amd.synthetic import CONFIGS, make_batch
from tests.helpers import (PPO_HP as HP, assert_grads, crowded as _crowded, device_batch as _batch, grad_report, make_pair, n_terms as _n_terms,
                           oracle_backward, rel_err, report_vs_float32 as _report_vs_float32)
from tests.test_gpu_covariant_deterministic import _autograd_vs_oracle, _step_grad

pytestmark = pytest.mark.gpu
REGIONS = (b'ord_cg', b'ord_phi', b'ord_dw')
GUARD = 4096


@pytest.fixture(autouse=True)
def _restore_switches(built_lib):
    from molgym_amd import _lib
    prev = (_lib.is_deterministic(), _lib.is_deterministic_covariant())
    yield
    _lib.set_deterministic(prev[0], covariant=prev[1])


def _ordered(on):
    import molgym_amd
    molgym_amd.set_deterministic(bool(on), covariant=bool(on))


def _finite_adv(d):
    """synthetic.make_batch normalises the advantages by their standard deviation: one sample alone gives 0 / 0"""
    if not np.isfinite(d['adv']).all():
        d['adv'] = np.linspace(0.7, -0.4, len(d['adv']))
    return d


def _shape(name, monkeypatch):
    """(agent, oracle, data, seed of the loss weights) of a shape of the module docstring"""
    if name == 'a':
        ac, ref, _ = make_pair('cfg4', seed=5)
        return ac, ref, _crowded('cfg4', [0, 1, 8, 9, 16, 17, 20], 11), 5
    if name in ('b1', 'b2'):
        monkeypatch.setitem(CONFIGS, 'cfg2_canvas8', dict(CONFIGS['cfg2'], canvas_size=8))
        ac, ref, _ = make_pair('cfg2_canvas8', seed=31)
        return ac, ref, _finite_adv(_crowded('cfg2_canvas8', [8] if name == 'b1' else [8, 1], 32)), 33
    if name == 'c':
        ac, ref, _ = make_pair('cfg2', seed=41, num_gaussians=8)
        return ac, ref, _crowded('cfg2', [7] * 260, 42), 43
    if name == 'd':
        from tests.test_gpu_wide_canvas import _batch as wide_batch, _cov_pair
        ac, ref, _ = _cov_pair(monkeypatch, 65, seed=65)
        return ac, ref, wide_batch(65, [0, 64, 65], seed=66), 67
    if name in ('e40', 'e41'):
        ac, ref, _ = make_pair('cfg4', seed=51)
        return ac, ref, _crowded('cfg4', [20] * int(name[1:]), 52), 53
    raise KeyError(name)


def _ws_bytes(ac, cfg):
    n = C.c_size_t(0)
    ac._chk(ac._L().mg_cov_workspace_bytes(C.byref(cfg), C.byref(n)))
    return n.value


def _regions(ac, cfg):
    """byte ranges of the three scratch regions of the ordered mode in a workspace of `cfg`"""
    out = []
    for name in REGIONS:
        off, cnt = C.c_int64(), C.c_int64()
        ac._chk(ac._L().mg_cov_workspace_lookup(C.byref(cfg), name, C.byref(off), C.byref(cnt)))
        out.append((4 * off.value, 4 * (off.value + cnt.value)))
    return out


def _poison(ac, cfg, byte):
    ws = ac._ws_cache[0]
    for b0, b1 in _regions(ac, cfg):
        assert 0 <= b0 < b1 <= ws.numel()
        ws[b0:b1].fill_(byte)


def _assert_poison_proof(ac, batch):
    """the step gives the bits of its first run whatever the three regions held before it"""
    s0, g0 = _step_grad(ac, batch)
    assert torch.isfinite(s0).all() and torch.isfinite(g0).all() and g0.abs().max().item() > 0
    for byte in (0x00, 0xFF, 0x7F):   # zeros, float32 NaN, about 3.4e38
        _poison(ac, batch.cfg, byte)
        s, g = _step_grad(ac, batch)
        assert torch.isfinite(s).all() and torch.isfinite(g).all(), hex(byte)
        assert torch.equal(s, s0) and torch.equal(g, g0), hex(byte)
    return s0, g0


def _worst_vs_oracle(ac, ref, data, seed):
    """({output: rel_err}, worst err / slot max over the parameter slots) of step + backward under the current switches"""
    B = len(data['obs'])
    g = torch.Generator().manual_seed(seed)
    w = tuple(torch.randn(B, generator=g, dtype=torch.float64) * s for s in (1.0, 0.3, 0.7))
    ac.theta.grad = None
    out = ac.step(data['obs'], data['act'])
    (out['logp'].double() * w[0].cuda() + out['ent'].double() * w[1].cuda() + out['v'].double() * w[2].cuda()).sum().backward()
    torch.cuda.synchronize()
    exp, want = oracle_backward(ref, data, w)
    report = grad_report(ac.theta.grad.detach().double().cpu(), want, ac.slot_table)
    return ({k: rel_err(out[k].detach(), exp[k].detach()) for k in ('logp', 'ent', 'v')},
            max(v[0] for v in report.values() if v[1] >= 1e-10))


def _three_repeats(ac, data):
    batch = _batch(ac, data)
    s0, g0 = _step_grad(ac, batch)
    assert torch.isfinite(g0).all() and g0.abs().max().item() > 0
    for _ in range(2):
        s, g = _step_grad(ac, batch)
        assert torch.equal(s, s0) and torch.equal(g, g0)


# ---- 2. poisoned scratch ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', ['a', 'b1', 'b2', 'c', 'd', 'e41'])
def test_poisoned_scratch_gives_the_same_bits(built_lib, monkeypatch, shape):
    ac, _, data, _ = _shape(shape, monkeypatch)
    _ordered(True)
    _assert_poison_proof(ac, _batch(ac, data))


@pytest.mark.parametrize('large,small', [('e41', [0, 1, 8, 9, 16, 17, 20]), ('c', [7, 0, 3, 7, 1])])
def test_stale_scratch_of_a_larger_step_is_not_read(built_lib, monkeypatch, large, small):
    """the largest shape, then a smaller one in the same cached workspace (its scratch regions now lie over what the larger step
    left there): the bits of the smaller step from NaN-filled regions"""
    ac, _, data, _ = _shape(large, monkeypatch)
    name = 'cfg4' if large == 'e41' else 'cfg2'
    _ordered(True)
    big, little = _batch(ac, data), _batch(ac, _crowded(name, small, 61))
    _step_grad(ac, big)
    ws = ac._ws_cache[0]
    s1, g1 = _step_grad(ac, little)
    assert ac._ws_cache[0] is ws   # (the same block)
    _poison(ac, big.cfg, 0xFF)
    _poison(ac, little.cfg, 0xFF)
    s2, g2 = _step_grad(ac, little)
    assert ac._ws_cache[0] is ws
    assert torch.isfinite(g1).all() and g1.abs().max().item() > 0
    assert torch.equal(s1, s2) and torch.equal(g1, g2)


# ---- 3. oracle parity at the new shapes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', ['b1', 'b2', 'c', 'd'])
def test_oracle_parity_at_the_new_shapes(built_lib, monkeypatch, shape):
    ac, ref, data, seed = _shape(shape, monkeypatch)
    _ordered(False)
    default = _worst_vs_oracle(ac, ref, data, seed)
    _ordered(True)
    ordered = _worst_vs_oracle(ac, ref, data, seed)
    print(f'\nshape {shape}: worst gradient slot (err / slot max) ordered {ordered[1]:.3e}  default {default[1]:.3e};  outputs ordered '
          f'{max(ordered[0].values()):.3e}  default {max(default[0].values()):.3e}')
    _autograd_vs_oracle(ac, ref, data, seed)


# ---- 4. guard bands and refusals ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ordered,shape', [(True, 'a'), (True, 'c'), (True, 'd'), (False, 'a'), (False, 'd')])
def test_workspace_of_exactly_the_reported_size(built_lib, monkeypatch, ordered, shape):
    ac, _, data, _ = _shape(shape, monkeypatch)
    _ordered(ordered)
    batch = _batch(ac, data)
    nbytes = _ws_bytes(ac, batch.cfg)
    big = torch.full((GUARD + nbytes + GUARD, ), 0xA5, dtype=torch.uint8, device='cuda')
    big[GUARD:GUARD + nbytes].zero_()
    ac.__dict__.pop('_ws_epoch', None)
    ac._ws_cache = {0: big[GUARD:GUARD + nbytes]}
    s, g = _step_grad(ac, batch)
    assert ac._ws_cache[0].data_ptr() == big.data_ptr() + GUARD and ac._ws_cache[0].numel() == nbytes
    assert torch.isfinite(s).all() and torch.isfinite(g).all() and g.abs().max().item() > 0
    assert bool((big[:GUARD] == 0xA5).all()) and bool((big[GUARD + nbytes:] == 0xA5).all())


def test_undersized_workspace_is_refused_untouched(built_lib, monkeypatch):
    """mg_cov_forward, called as _CovStep.forward calls it, with the switch on and a buffer sized with the switch off -- and with one
    256-byte granule less than the ordered size"""
    from molgym_amd import _lib
    from molgym_amd.agents.covariant import _ptr, _stream
    ac, _, data, _ = _shape('a', monkeypatch)
    _ordered(False)
    batch = _batch(ac, data)
    n_off = _ws_bytes(ac, batch.cfg)
    _ordered(True)
    n_on = _ws_bytes(ac, batch.cfg)
    assert n_on % 256 == 0 and n_on - 256 > n_off
    lib = ac._L()
    out = torch.zeros(3, batch.cfg.B, dtype=torch.float32, device='cuda')
    for nbytes in (n_off, n_on - 256):
        buf = torch.full((nbytes, ), 0xA5, dtype=torch.uint8, device='cuda')
        with pytest.raises(RuntimeError, match=str(n_on)):
            _lib.check(lib.mg_cov_forward(C.byref(batch.cfg), _ptr(ac._ktheta()), _ptr(batch.pos), _ptr(batch.charges), _ptr(batch.bags),
                                          _ptr(batch.actions), _ptr(ac.leb), _ptr(buf), nbytes, _ptr(out), _stream(ac.theta.device)), lib)
        torch.cuda.synchronize()
        assert bool((buf == 0xA5).all()), nbytes


def test_forward_ordered_backward_not_is_refused(built_lib, monkeypatch):
    """the mirror of the forward-off / backward-on refusal of tests/test_gpu_covariant_deterministic.py"""
    ac, _, cfg = make_pair('cfg2', seed=3)
    data = make_batch(6, cfg['canvas_size'], cfg['zs'], seed=2)
    _ordered(True)
    out = ac.step(data['obs'], data['act'])
    _ordered(False)
    before = torch.full_like(ac.theta, 0.25)
    ac.theta.grad = before.clone()
    with pytest.raises(RuntimeError):
        out['logp'].sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(ac.theta.grad, before)


# ---- 5. the 16 384-edge layout boundary ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', ['e40', 'e41'])
def test_ordered_against_default_across_the_layout_boundary(built_lib, monkeypatch, shape):
    """the default mode is held to float64 at this size family by tests/test_gpu_large.py and the two modes sum the same terms in
    another order: the project's own gradient bounds, with the default-mode gradient of a copy of the agent as the reference"""
    ac, _, data, _ = _shape(shape, monkeypatch)
    assert sum(len([1 for it in o[0] if it[0] != 0]) ** 2 for o in data['obs']) == (16000 if shape == 'e40' else 16400)
    other = copy.deepcopy(ac)
    _ordered(False)
    sd, gd = _step_grad(other, _batch(other, data))
    _ordered(True)
    batch = _batch(ac, data)
    s0, g0 = _step_grad(ac, batch)
    for _ in range(2):
        s, g = _step_grad(ac, batch)
        assert torch.equal(s, s0) and torch.equal(g, g0)
    assert torch.isfinite(g0).all() and torch.isfinite(s0).all() and torch.isfinite(sd).all()
    report = _report_vs_float32(g0, gd, ac.slot_table, _n_terms(data))
    print(f'\nshape {shape}: worst gradient slot, ordered against default (err / slot max):', max(v[0] for v in report.values() if v[1] >= 1e-10))
    assert_grads(report)


@pytest.mark.parametrize('first_ordered', [False, True])
def test_switch_flip_between_two_minibatches_of_an_epoch(built_lib, monkeypatch, first_ordered):
    """41 full canvases (the two modes lay the workspace out differently), one agent, one cached slot, no invalidate_weights()
    between the steps: a default-mode and an ordered epoch-cached step, in either order, on ONE block that is large enough for
    both (so the second step carries the first one's weights claim and, default first, finds its deferred fold pending), then the
    fold.  Either the second step refuses or theta.grad is the sum of the two gradients taken alone; and the agent is fit for a
    plain default step afterwards."""
    base, _, data, _ = _shape('e41', monkeypatch)
    alone = {}
    for mode in (False, True):
        one = copy.deepcopy(base)
        _ordered(mode)
        alone[mode] = _step_grad(one, _batch(one, data))[1]
    ac = copy.deepcopy(base)
    batch = _batch(ac, data)
    # the slot's block is obtained while the switch is on: large enough for both modes (a block of the default size plus its
    # headroom is smaller than the ordered size here and would be REPLACED at the flip, which is another, older path)
    _ordered(True)
    ws = ac._workspace(batch.cfg)
    assert ws.numel() >= _ws_bytes(ac, batch.cfg)
    _ordered(False)
    assert ws.numel() >= _ws_bytes(ac, batch.cfg)
    ac.theta.grad = torch.zeros_like(ac.theta)
    ac.invalidate_weights()
    seen = []   # (block, does the slot claim current weights) as each step got them from _workspace()
    inner = ac._workspace

    def spy(cfg, slot=0, epoch_step=False):
        block = inner(cfg, slot, epoch_step)
        seen.append((block, bool(ac.__dict__.get('_ws_epoch', {}).get(slot, {}).get('weights'))))
        return block

    monkeypatch.setattr(ac, '_workspace', spy)
    _ordered(first_ordered)
    ac.ppo_minibatch(batch, *HP, epoch_cache=True)
    _ordered(not first_ordered)
    raised = False
    try:
        ac.ppo_minibatch(batch, *HP, epoch_cache=True)
    except RuntimeError:
        raised = True
    monkeypatch.setattr(ac, '_workspace', inner)
    # one cached block under both layouts, and the second step carried the first one's claim (MG_STEP_WEIGHTS_CURRENT) over it
    print('\nblocks the same:', seen[0][0] is ws and seen[1][0] is ws, ' weights claimed at step 1 / 2:', seen[0][1], seen[1][1])
    assert len(seen) == 2 and seen[0][0] is ws and seen[1][0] is ws and ac._ws_cache[0] is ws
    assert seen[0][1] is False and seen[1][1] is True
    ac.fold_gradients()
    torch.cuda.synchronize()
    print('\nsecond step after the flip:', 'refused' if raised else 'ran')
    assert torch.isfinite(ac.theta.grad).all()
    if not raised:
        report = _report_vs_float32(ac.theta.grad, alone[False] + alone[True], ac.slot_table, _n_terms(data))
        print('worst gradient slot against the sum of the two alone:', max(v[0] for v in report.values() if v[1] >= 1e-10))
        assert_grads(report)
    _ordered(False)
    ac.invalidate_weights()
    _, g = _step_grad(ac, batch)
    assert_grads(_report_vs_float32(g, alone[False], ac.slot_table, _n_terms(data)))


# ---- 6. other builds and configurations in the mode ---------------------------------------------------------------------------
def _variant(name, monkeypatch):
    """(agent, oracle, data, seed of the loss weights): the small cases of the default-mode tests that cover the same variants"""
    if name == 'zs16':   # tests/test_gpu_wide_zs.py: COV_CASES[2]
        from tests.test_gpu_wide_zs import _batch as zs_batch, _cov_pair
        ac, ref, _ = _cov_pair(monkeypatch, 16, 6, seed=42)
        return ac, ref, zs_batch(16, 6, [6, 0, 1, 5], seed=43), 44
    kw, seed, B, dseed, wseed = {
        'channels_8_2': (dict(num_channels_hidden=8, num_channels_per_element=2), 21, 12, 33, 2),  # test_other_channel_counts_vs_oracle
        'channels_7_3': (dict(num_channels_hidden=7, num_channels_per_element=3), 173, 12, 33, 2),  # test_gpu_channel_builds.py, shape S
        'cg_levels_4': (dict(num_cg_levels=4), 27, 6, 35, 3),
        'width_256': (dict(network_width=256), 23, 24, 37, 4),                                      # test_network_width_256_vs_oracle
        'no_beta': (dict(beta=None), 3, 12, 6, 3),                                                  # test_gpu_backward.py::test_grads_no_beta
        'maxl_2': (dict(maxl=2), 29, 12, 39, 5),                                                    # test_other_maxl_vs_oracle[2]
    }[name]
    ac, ref, cfg = make_pair('cfg2', seed=seed, **kw)
    return ac, ref, make_batch(B, cfg['canvas_size'], cfg['zs'], seed=dseed), wseed


@pytest.mark.parametrize('variant', ['channels_8_2', 'channels_7_3', 'cg_levels_4', 'width_256', 'no_beta', 'zs16', 'maxl_2'])
def test_other_builds_and_configurations_in_the_mode(built_lib, monkeypatch, variant):
    from molgym_amd import _lib
    ac, ref, data, wseed = _variant(variant, monkeypatch)
    _ordered(True)
    if variant in ('channels_8_2', 'channels_7_3', 'cg_levels_4'):
        assert ac._L() is not _lib.lib() and ac._L().mg_cov_get_ordered() == 1   # (variant libraries follow both switches)
    _autograd_vs_oracle(ac, ref, data, wseed)
    _three_repeats(ac, data)
