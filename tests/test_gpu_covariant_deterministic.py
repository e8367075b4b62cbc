"""CovariantAC's ordered mode (molgym_amd.set_deterministic(True, covariant=True)): the training forward, the backward and the PPO
mini-batch step give the same bits on every run and however the step is issued, and still agree with the float64 oracle to the
project's own tolerances (tests/helpers.py: rel_err < 1e-5 on the outputs, assert_grads on every parameter gradient).

Cases: (a) cfg2, B = 33 -- by default the fused heads, the fused level 0 and the fused edge levels, all of which the mode leaves;
(b) cfg4, the crowded canvases [20, 17, 19] of tests/test_gpu_parity_full.py::test_canvas20_crowded_vs_oracle (same weights, inputs
and loss weights: the session's oracle cache serves it); (c) cfg4 with 0, 1, 8, 9, 16, 17 and 20 atoms -- an empty sample, a single
atom, an exact tile of 8 neighbours, a tile plus one, an exact tile of 16 of the level-0 kernel, two tiles plus one, a full canvas;
(d) cfg2 at B = 140 (repeat test only)."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from molgym_amd.synthetic import make_batch
from tests.helpers import PPO_HP as HP, assert_grads, crowded as _crowded, device_batch as _batch, grad_report, make_pair, oracle_backward, rel_err

pytestmark = pytest.mark.gpu
CASES = ['a', 'b', 'c']


@pytest.fixture(autouse=True)
def _restore_switches(built_lib):
    from molgym_amd import _lib
    prev = (_lib.is_deterministic(), _lib.is_deterministic_covariant())
    yield
    _lib.set_deterministic(prev[0], covariant=prev[1])


def _case(case):
    """(cfg name, agent seed, data) of a case"""
    if case == 'a':
        return 'cfg2', 0, make_batch(33, 7, [0, 9, 16], seed=3)
    if case == 'b':
        return 'cfg4', 7, _crowded('cfg4', [20, 17, 19], 7)
    if case == 'c':
        return 'cfg4', 5, _crowded('cfg4', [0, 1, 8, 9, 16, 17, 20], 11)
    if case == 'd':
        return 'cfg2', 0, make_batch(140, 7, [0, 9, 16], seed=3)
    raise KeyError(case)


def _step_grad(ac, batch, **kw):
    ac.theta.grad = torch.zeros_like(ac.theta)
    stats = ac.ppo_minibatch(batch, *HP, **kw)
    torch.cuda.synchronize()
    return stats.clone(), ac.theta.grad.clone()


def _autograd_vs_oracle(ac, ref, data, seed):
    B = len(data['obs'])
    g = torch.Generator().manual_seed(seed)
    wl, we, wv = (torch.randn(B, generator=g, dtype=torch.float64) * s for s in (1.0, 0.3, 0.7))
    ac.theta.grad = None
    out = ac.step(data['obs'], data['act'])
    (out['logp'].double() * wl.cuda() + out['ent'].double() * we.cuda() + out['v'].double() * wv.cuda()).sum().backward()
    torch.cuda.synchronize()
    exp, want = oracle_backward(ref, data, (wl, we, wv))
    for k in ('logp', 'ent', 'v'):
        err = rel_err(out[k].detach(), exp[k].detach())
        print(k, err)
        assert err < 1e-5, (k, err)
    report = grad_report(ac.theta.grad.detach().double().cpu(), want, ac.slot_table)
    print('worst gradient slot (err / slot max):', max(v[0] for v in report.values() if v[1] >= 1e-10))
    assert_grads(report)


@pytest.mark.parametrize('case', CASES)
def test_oracle_parity_in_the_mode(built_lib, case):
    import molgym_amd
    name, seed, data = _case(case)
    ac, ref, _ = make_pair(name, seed=seed)
    molgym_amd.set_deterministic(True, covariant=True)
    _autograd_vs_oracle(ac, ref, data, seed)


@pytest.mark.parametrize('case', CASES + ['d'])
def test_same_bits_on_every_run_and_in_every_form(built_lib, case):
    import molgym_amd
    from molgym_amd import _lib
    name, seed, data = _case(case)
    ac, _, cfg = make_pair(name, seed=seed)
    molgym_amd.set_deterministic(True, covariant=True)
    batch = _batch(ac, data)
    B = len(data['obs'])
    # five runs from a zeroed gradient
    s0, g0 = _step_grad(ac, batch, graph=False)
    assert torch.isfinite(g0).all() and g0.abs().max().item() > 0
    for _ in range(4):
        s, g = _step_grad(ac, batch, graph=False)
        assert torch.equal(s, s0) and torch.equal(g, g0)
    # graph requested == not requested (an ordered step is issued as stream launches either way)
    s, g = _step_grad(ac, batch, graph=True)
    assert torch.equal(s, s0) and torch.equal(g, g0) and ac.last_step_used_graph is False
    # epoch cache (derived weights kept, MG_STEP_DEFER_FOLD) on against off, over ragged mini-batches through one cached workspace
    n = len(data['obs'])
    cuts = [list(range(n)), list(range(0, n, 2)), [n - 1], list(range(n - 1, -1, -1))]
    batches = [_batch(ac, {'obs': [data['obs'][i] for i in ix], **{k: np.asarray(data[k])[ix] for k in ('act', 'logp', 'adv', 'ret')}})
               for ix in cuts]
    res = {}
    for cached in (False, True):
        ac.theta.grad = torch.zeros_like(ac.theta)
        ac.invalidate_weights()
        acc = torch.zeros(6, dtype=torch.float64, device='cuda')
        outs = [ac.ppo_minibatch(b, *HP, loss_scale=0.5, stats_accum=acc, epoch_cache=cached).clone() for b in batches]
        if cached:
            ac.fold_gradients()
        torch.cuda.synchronize()
        res[cached] = (outs, ac.theta.grad.clone(), acc.clone())
    for x, y in zip(res[False][0], res[True][0]):
        assert torch.equal(x, y)
    assert torch.equal(res[False][1], res[True][1]) and torch.equal(res[False][2], res[True][2])
    # step(obs, actions) + backward() fed the loss kernel's own gout == ppo_minibatch (the form of
    # tests/test_gpu_internal_deterministic.py::test_autograd_path_equals_the_fused_step)
    ac.theta.grad = None
    out = ac.step(data['obs'], data['act'])
    pred = torch.stack([out['logp'], out['ent'], out['v']]).detach().contiguous()
    gout = torch.empty(3, B, dtype=torch.float32, device='cuda')
    stats2 = torch.empty(6, dtype=torch.float64, device='cuda')
    P = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(built_lib.mg_ppo_loss(B, P(pred), P(batch.logp), P(batch.adv), P(batch.ret), HP[0], HP[1], HP[2], P(stats2), P(gout),
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.autograd.backward([out['logp'], out['ent'], out['v']], [gout[0], gout[1], gout[2]])
    torch.cuda.synchronize()
    assert torch.equal(stats2, s0) and torch.equal(ac.theta.grad, g0)
    # three more runs while a second stream keeps the chip busy with matmuls: workgroup placement differs
    side = torch.cuda.Stream()
    m = torch.randn(2048, 2048, device='cuda')
    side.wait_stream(torch.cuda.current_stream())
    for _ in range(3):
        with torch.cuda.stream(side):
            for _ in range(6):
                m2 = m @ m
        s, g = _step_grad(ac, batch, graph=False)
        assert torch.equal(s, s0) and torch.equal(g, g0)
    side.synchronize()
    del m2


def test_sensitivity_control_default_mode_varies(built_lib):
    """a repeat test proves nothing if the default mode repeats at that shape too: case (b) ten times with both switches off.
    Never asserts that the default mode differs; skips when it saw no variation."""
    import molgym_amd
    name, seed, data = _case('b')
    ac, _, _ = make_pair(name, seed=seed)
    molgym_amd.set_deterministic(False)
    batch = _batch(ac, data)
    seen = set()
    for _ in range(10):
        _, g = _step_grad(ac, batch, graph=False)
        seen.add(g.cpu().numpy().tobytes())
    print('distinct default-mode gradients in ten runs:', len(seen))
    if len(seen) < 2:
        pytest.skip('the control saw no variation: the default mode repeated its bits ten times at this shape')


def test_wide_canvas_large_list_build_repeats(built_lib):
    """wide128, B = 2 with 70 and 128 atoms: staged heads by default, the large list build (whose descriptor slots are handed out
    by integer atomics, in an order that varies) and 21 284 edges, above the default threshold of the shared DotMatrix layout"""
    import molgym_amd
    ac, _, cfg = make_pair('wide128', seed=2)
    data = _crowded('wide128', [70, 128], 4)
    molgym_amd.set_deterministic(True, covariant=True)
    batch = _batch(ac, data)
    s0, g0 = _step_grad(ac, batch)
    assert torch.isfinite(g0).all() and g0.abs().max().item() > 0
    for _ in range(2):
        s, g = _step_grad(ac, batch)
        assert torch.equal(s, s0) and torch.equal(g, g0)


def test_other_num_cg_levels_build(built_lib):
    """the num_cg_levels = 2 build of the same sources: oracle parity and repeats on cfg2, B = 6"""
    import molgym_amd
    ac, ref, cfg = make_pair('cfg2', seed=27, num_cg_levels=2)
    data = make_batch(6, cfg['canvas_size'], cfg['zs'], seed=35)
    molgym_amd.set_deterministic(True, covariant=True)
    assert ac._L().mg_cov_get_ordered() == 1  # (variant libraries follow both switches)
    _autograd_vs_oracle(ac, ref, data, 3)
    batch = _batch(ac, data)
    s0, g0 = _step_grad(ac, batch)
    for _ in range(2):
        s, g = _step_grad(ac, batch)
        assert torch.equal(s, s0) and torch.equal(g, g0)


def test_train_twice_gives_the_same_bits(built_lib):
    """24 samples in mini-batches of 12, two epochs, twice from copies of one agent.  The recorded log-probs sit 0.05 above the agent's
    own (ratios near one: nothing is clipped away)."""
    import molgym_amd
    from molgym_amd import ppo
    base, _, cfg = make_pair('cfg2', seed=12)
    data = make_batch(24, cfg['canvas_size'], cfg['zs'], seed=21)
    with torch.no_grad():
        data['logp'] = base.step(data['obs'], data['act'])['logp'].double().cpu().numpy() + 0.05
    molgym_amd.set_deterministic(True, covariant=True)
    runs = []
    for _ in range(2):
        ac = copy.deepcopy(base)
        opt = torch.optim.Adam(ac.parameters(), lr=3e-4)
        np.random.seed(5)
        infos = ppo.train(ac, opt, data, mini_batch_size=12, clip_ratio=0.2, target_kl=1e9, vf_coef=0.5, entropy_coef=0.01,
                          gradient_clip=0.5, max_num_steps=2)
        torch.cuda.synchronize()
        st = opt.state.get(ac.theta, {})
        runs.append((infos, ac.theta.detach().clone(), st.get('exp_avg'), st.get('exp_avg_sq')))
    a, b = runs
    assert a[0]['num_opt_steps'] == b[0]['num_opt_steps'] == 2
    assert set(a[0]) == set(b[0])
    for k in a[0]:
        if k != 'time':
            assert a[0][k] == b[0][k], (k, a[0][k], b[0][k])
    assert torch.equal(a[1], b[1]) and not torch.equal(a[1], base.theta.detach())
    assert a[2] is not None and a[3] is not None
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


def test_switch_semantics_on_the_device(built_lib):
    import molgym_amd
    ac, _, cfg = make_pair('cfg2', seed=3)
    data = make_batch(6, cfg['canvas_size'], cfg['zs'], seed=2)
    batch = _batch(ac, data)
    ac.ppo_minibatch(batch, *HP)
    torch.cuda.synchronize()
    graph_before = ac.last_step_used_graph
    # the first switch alone still refuses (tests/test_gpu_internal_deterministic.py::test_covariant_agent_refuses pins it)
    molgym_amd.set_deterministic(True)
    with pytest.raises(RuntimeError, match='deterministic mode covers SchNetAC only'):
        ac.ppo_minibatch(batch, *HP)
    # a forward with the second switch off, a backward with it on: refused, not run on a layout that is not there
    molgym_amd.set_deterministic(False)
    out_off = ac.step(data['obs'], data['act'])
    molgym_amd.set_deterministic(True, covariant=True)
    assert molgym_amd.is_deterministic() and molgym_amd.is_deterministic_covariant()
    with pytest.raises(RuntimeError):
        out_off['logp'].sum().backward()
    # with both on, both entry points run
    ac.theta.grad = None
    stats = ac.ppo_minibatch(batch, *HP)
    out = ac.step(data['obs'], data['act'])
    out['logp'].sum().backward(retain_graph=True)
    torch.cuda.synchronize()
    assert torch.isfinite(stats).all() and torch.isfinite(ac.theta.grad).all() and ac.last_step_used_graph is False
    # set_deterministic(True) without the keyword turns the second switch off again: the agent refuses, both ways
    molgym_amd.set_deterministic(True)
    assert not molgym_amd.is_deterministic_covariant()
    with pytest.raises(RuntimeError, match='deterministic mode covers SchNetAC only'):
        ac.ppo_minibatch(batch, *HP)
    with pytest.raises(RuntimeError, match='deterministic mode covers SchNetAC only'):
        out['v'].sum().backward()
    # everything off: the default step, issued as it was before
    molgym_amd.set_deterministic(False)
    ac.theta.grad = None
    ac.ppo_minibatch(batch, *HP)
    torch.cuda.synchronize()
    assert torch.isfinite(ac.theta.grad).all() and ac.last_step_used_graph == graph_before
