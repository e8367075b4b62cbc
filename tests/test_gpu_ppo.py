"""PPO loss / GAE / normalisation / clip kernels against the reference-generated golden vectors, and the
train() driver against the oracle's autograd-based restatement of the same loop."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from molgym_amd import _lib
from molgym_amd.synthetic import make_batch
from tests.helpers import make_pair

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), 'golden')
P = lambda t: C.c_void_p(t.data_ptr())
S = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)


def test_ppo_loss_kernel_matches_reference(built_lib):
    g = np.load(os.path.join(G, 'g1_compute_loss.npz'))
    for B in (1, 7, 140):
        pred = torch.tensor(np.stack([g[f'B{B}_logp'], g[f'B{B}_ent'], g[f'B{B}_v']])).cuda()
        old, adv, ret = (torch.tensor(g[f'B{B}_{k}']).cuda() for k in ('old_logp', 'adv', 'ret'))
        stats = torch.empty(6, dtype=torch.float64, device='cuda')
        gout = torch.empty(3, B, dtype=torch.float32, device='cuda')
        _lib.check(built_lib.mg_ppo_loss(B, P(pred), P(old), P(adv), P(ret), 0.2, 0.5, 0.01, P(stats), P(gout), S()))
        got, want = stats.cpu().numpy(), g[f'B{B}_stats']
        # the reference takes the entropy mean in float32 (pred['ent'] is float32); the kernel sums in float64
        # and the clip fraction is a float32 mean there (ppo.py:52)
        np.testing.assert_allclose(got[[0, 2, 4]], want[[0, 2, 4]], rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(got[[1, 3, 5]], want[[1, 3, 5]], rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(gout.cpu().numpy(), g[f'B{B}_grads'], rtol=1e-6, atol=1e-12)


def test_gae_and_adv_normalise_kernels_match_reference(built_lib):
    g = np.load(os.path.join(G, 'g2_gae.npz'))
    for c in (0, 1):
        off = torch.tensor(g[f'c{c}_off']).cuda()
        rew, val, last = (torch.tensor(g[f'c{c}_{k}']).cuda() for k in ('rew', 'val', 'last'))
        adv, ret = torch.empty_like(rew), torch.empty_like(rew)
        _lib.check(built_lib.mg_gae(len(g[f'c{c}_last']), P(off), P(rew), P(val), P(last), float(g[f'c{c}_gamma']),
                                    float(g[f'c{c}_lam']), P(adv), P(ret), S()))
        np.testing.assert_allclose(adv.cpu().numpy(), g[f'c{c}_adv'], rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(ret.cpu().numpy(), g[f'c{c}_ret'], rtol=1e-12, atol=1e-14)
        _lib.check(built_lib.mg_adv_normalize(adv.numel(), P(adv), None, S()))
        np.testing.assert_allclose(adv.cpu().numpy(), g[f'c{c}_adv_norm'], rtol=1e-11, atol=1e-13)


def test_grad_norm_and_clip(built_lib):
    torch.manual_seed(0)
    gref = torch.randn(185006)
    for max_norm in (0.5, 1e6):
        gdev = gref.clone().cuda()
        out = torch.zeros(2, device='cuda')
        _lib.check(built_lib.mg_grad_norm_clip(gdev.numel(), P(gdev), max_norm, P(out), S()))
        p = torch.nn.Parameter(torch.zeros_like(gref))
        p.grad = gref.clone()
        norm = torch.nn.utils.clip_grad_norm_([p], max_norm)
        assert abs(out[0].item() - norm.item()) / norm.item() < 1e-5
        assert torch.allclose(gdev.cpu(), p.grad, rtol=1e-5, atol=1e-7)


def test_grad_norm_kernel_against_the_reference_value(built_lib):
    """G9: util.compute_gradient_norm of the reference (tools/util.py:61-69) on the gradients of G4's MLP, stored by
    oracle/make_golden.py as g4['grad_norm']; mg_grad_norm_clip reports the same norm from the flat gradient."""
    import os
    g = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'g4_mlp.npz'))
    flat = torch.cat([torch.tensor(g[k]).reshape(-1) for k in g.files if k.startswith('grad_') and k != 'grad_norm']).cuda()
    keep = flat.clone()
    out = torch.zeros(2, device='cuda')
    _lib.check(built_lib.mg_grad_norm_clip(flat.numel(), P(flat), 1e9, P(out), S()))
    want = float(g['grad_norm'])
    assert abs(out[0].item() - want) <= 1e-6 * want
    assert torch.equal(flat, keep)  # far below the limit: untouched


def test_fused_minibatch_equals_autograd_path(built_lib):
    """ppo_minibatch (device loss + hand-written backward) == compute_loss through autograd == oracle."""
    from molgym_amd import ppo
    from oracle.ppo_ref import compute_loss_ref
    ac, ref, cfg = make_pair('cfg2', seed=21)
    data = make_batch(32, cfg['canvas_size'], cfg['zs'], seed=8)
    batch = ac.prepare_batch(data['obs'], data['act'], data['logp'], data['adv'], data['ret'])
    stats = ac.ppo_minibatch(batch, 0.2, 0.5, 0.01)
    g_fast = ac.theta.grad.clone()
    ac.theta.grad = None
    loss, info = ppo.compute_loss(ac, data, 0.2, 0.5, 0.01)
    loss.backward()
    g_auto = ac.theta.grad.clone()
    rloss, rinfo = compute_loss_ref(ref, data, 0.2, 0.5, 0.01, step_dtype=torch.float64)
    rloss.backward()
    for i, k in enumerate(ppo.KEYS):
        assert abs(stats[i].item() - rinfo[k]) < 1e-5 * max(1.0, abs(rinfo[k])), k
        assert abs(info[k] - rinfo[k]) < 1e-5 * max(1.0, abs(rinfo[k])), k
    scale = g_auto.abs().max().item()
    assert (g_fast - g_auto).abs().max().item() < 1e-4 * scale
    want = dict(ref.named_parameters())
    for name, (off, shape) in ac.slot_table.items():
        n = int(np.prod(shape))
        gw = want[name].grad.reshape(-1)
        sc = max(gw.abs().max().item(), 1e-12)
        assert ((g_fast[off:off + n].double().cpu() - gw).abs().max().item() / sc) < 2e-4 or sc < 1e-10, name


def test_train_loop_matches_oracle_loop(built_lib):
    """Two epochs of ppo.train (mini-batches of 16 over a 40-step rollout incl. a remainder batch) track the
    same loop run with the oracle + torch Adam on the CPU."""
    from molgym_amd import ppo
    from oracle.ppo_ref import batch_indices_ref, compute_loss_ref
    ac, ref, cfg = make_pair('cfg2', seed=22)
    data = make_batch(40, cfg['canvas_size'], cfg['zs'], seed=10)
    data['logp'] = data['logp'] * 0 + ac.step(data['obs'], data['act'])['logp'].detach().double().cpu().numpy() - 0.001
    opt = torch.optim.Adam(ac.parameters(), lr=3e-4)
    ropt = torch.optim.Adam(ref.parameters(), lr=3e-4)
    np.random.seed(5)
    infos = ppo.train(ac, opt, data, mini_batch_size=16, clip_ratio=0.2, target_kl=1e9, vf_coef=0.5, entropy_coef=0.01,
                      gradient_clip=0.5, max_num_steps=2)
    np.random.seed(5)
    for _ in range(2):
        ropt.zero_grad()
        stats = []
        for idx in batch_indices_ref(40, 16):
            sub = ppo.collect_data_batch(data, idx)
            loss, info = compute_loss_ref(ref, sub, 0.2, 0.5, 0.01, step_dtype=torch.float64)
            loss.backward()
            stats.append(info)
        torch.nn.utils.clip_grad_norm_(ref.parameters(), 0.5)
        ropt.step()
    assert infos['num_opt_steps'] == 2
    mean = ppo.compute_mean_dict(stats)
    for k in ppo.KEYS:
        assert abs(infos[k] - mean[k]) < 2e-4 * max(1.0, abs(mean[k])), (k, infos[k], mean[k])
    new = ac.export_state_dict()
    for k, v in ref.state_dict().items():
        d = (new[k].double().cpu() - v).abs().max().item()
        assert d < 1e-4, (k, d)  # two Adam steps of lr 3e-4


def test_graph_step_equals_stream_launches(built_lib):
    """mg_cov_ppo_step as ONE updated hipGraph launch == the same step as ~27 stream launches: statistics, step outputs and
    gradient of single mini-batches of DIFFERENT ragged sizes replayed through the same cached graph (every replay updates all
    kernel nodes: grids and arguments follow TA / TE), and theta after two epochs of ppo.train (three mini-batches in flight,
    one graph per stream slot) to the run-to-run reproducibility of the float atomics (2e-5)."""
    from molgym_amd import ppo
    ac, ref, cfg = make_pair('cfg2', seed=24)
    sizes = (24, 31, 9, 24)
    batches = []
    for k, B in enumerate(sizes):
        d = make_batch(B, cfg['canvas_size'], cfg['zs'], seed=40 + k)
        batches.append(ac.prepare_batch(d['obs'], d['act'], d['logp'], d['adv'], d['ret']))
    for b in batches:  # several sizes through ONE cached graph (slot 0)
        res = {}
        for mode in (False, True):
            ac.theta.grad = torch.zeros_like(ac.theta)
            acc = torch.zeros(6, dtype=torch.float64, device='cuda')
            stats = ac.ppo_minibatch(b, 0.2, 0.5, 0.01, loss_scale=0.5, stats_accum=acc, graph=mode)
            torch.cuda.synchronize()
            assert ac.last_step_used_graph == mode
            res[mode] = (stats.clone(), ac._last_out.clone(), ac.theta.grad.clone(), acc.clone())
        (s0, o0, g0, a0), (s1, o1, g1, a1) = res[False], res[True]
        assert torch.equal(s0, s1) and torch.equal(o0, o1)       # forward + loss: no atomics, bit for bit
        assert torch.allclose(a1, 0.5 * s1, rtol=1e-14, atol=0)  # the epoch accumulator got share x statistics
        assert (g0 - g1).abs().max().item() <= 2e-5 * g0.abs().max().item()
    # the training loop, both ways
    data = make_batch(60, cfg['canvas_size'], cfg['zs'], seed=50)
    theta0 = ac.theta.detach().clone()
    out = {}
    for mode in (False, True):
        with torch.no_grad():
            ac.theta.copy_(theta0)
        ac.use_graphs = mode
        # (SGD: linear in the gradient.  Adam's step is ~ lr g / |g| per entry: where g ~ 0 the run-to-run order of the float atomics
        # decides a sign and the two runs part by up to 2 lr -- the round-6 run failed this comparison at 8.8e-5 with no kernel of the
        # step changed in what it computes)
        opt = torch.optim.SGD(ac.parameters(), lr=0.05)
        np.random.seed(6)
        info = ppo.train(ac, opt, data, mini_batch_size=16, clip_ratio=0.2, target_kl=1e9, vf_coef=0.5, entropy_coef=0.01,
                         gradient_clip=0.5, max_num_steps=2)
        assert ac.last_step_used_graph == mode
        out[mode] = (ac.theta.detach().clone(), info)
    ac.use_graphs = True
    d = (out[True][0] - out[False][0]).abs().max().item()
    assert d <= 2e-5 * out[False][0].abs().max().item(), d
    for k in ppo.KEYS:
        assert abs(out[True][1][k] - out[False][1][k]) <= 1e-6 * max(1.0, abs(out[False][1][k])), k


def test_epoch_cache_equals_per_minibatch_preparation(built_lib):
    """What depends on theta alone, once per EPOCH (mg_cov_ppo_step flags MG_STEP_WEIGHTS_CURRENT / MG_STEP_DEFER_FOLD +
    mg_cov_fold_grads; theta is constant over an epoch's mini-batches, ppo.py:117-146) == the same mini-batches each preparing the
    derived weights and folding the expanded weight gradients itself: per-step statistics and outputs bit for bit, the epoch's
    gradient to the reproducibility of its float atomics -- for mini-batches of different ragged sizes through ONE workspace
    (the derived weights sit at batch-independent offsets), graph and stream form, and across a change of theta."""
    ac, ref, cfg = make_pair('cfg2', seed=31)
    sizes = (24, 31, 9, 140, 24)
    batches = []
    for k, B in enumerate(sizes):
        d = make_batch(B, cfg['canvas_size'], cfg['zs'], seed=70 + k)
        batches.append(ac.prepare_batch(d['obs'], d['act'], d['logp'], d['adv'], d['ret']))
    for graph in (True, False):
        for epoch in range(2):
            res = {}
            for cached in (False, True):
                ac.theta.grad = torch.zeros_like(ac.theta)
                ac.invalidate_weights()
                outs = []
                for b in batches:
                    st = ac.ppo_minibatch(b, 0.2, 0.5, 0.01, loss_scale=0.5, graph=graph, epoch_cache=cached)
                    outs.append((st.clone(), ac._last_out.clone()))
                if cached:
                    state = ac._ws_epoch[0]
                    assert state['weights'] and state['pending']
                    ac.fold_gradients()
                    assert not ac._ws_epoch[0]['pending']
                torch.cuda.synchronize()
                res[cached] = (outs, ac.theta.grad.clone())
            for (s0, o0), (s1, o1) in zip(res[False][0], res[True][0]):
                assert torch.equal(s0, s1) and torch.equal(o0, o1)
            g0, g1 = res[False][1], res[True][1]
            assert torch.isfinite(g1).all() and (g0 - g1).abs().max().item() <= 2e-5 * g0.abs().max().item()
            # every slot of the gradient is there (a missing fold would leave the complex mixes' slots at zero)
            for name, (off, shape) in ac.slot_table.items():
                n = int(np.prod(shape))
                if g0[off:off + n].abs().max().item() > 0:
                    assert g1[off:off + n].abs().max().item() > 0, name
            with torch.no_grad():  # "the optimizer steps": the next epoch must see the new theta
                ac.theta.add_(0.01 * torch.randn_like(ac.theta))


def test_runahead_epochs_equal_synchronous_loop(built_lib, monkeypatch):
    """ppo.train with the KL test / norm / clip on the device and the next epoch issued before the previous one's record is read
    (molgym_amd/ppo.py::_train_runahead) == the loop that synchronises every epoch like the reference (ppo.py:133-146): same
    number of optimizer steps when the KL test fires in the middle, same theta, same statistics, same Adam step counter, and
    the numpy RNG left where the reference's loop leaves it (the speculative epoch's permutation is taken back)."""
    from molgym_amd import ppo
    ac, ref, cfg = make_pair('cfg2', seed=25)
    data = make_batch(48, cfg['canvas_size'], cfg['zs'], seed=60)
    data['logp'] = data['logp'] * 0 + ac.step(data['obs'], data['act'])['logp'].detach().double().cpu().numpy()
    theta0 = ac.theta.detach().clone()

    def run(mode, target_kl, max_steps=6):
        monkeypatch.setenv('MOLGYM_RUNAHEAD', mode)
        with torch.no_grad():
            ac.theta.copy_(theta0)
        ac.theta.grad = None
        opt = torch.optim.Adam(ac.parameters(), lr=3e-4)
        np.random.seed(7)
        info = ppo.train(ac, opt, data, mini_batch_size=16, clip_ratio=0.2, target_kl=target_kl, vf_coef=0.5, entropy_coef=0.01,
                         gradient_clip=0.5, max_num_steps=max_steps)
        st = opt.state[ac.theta]
        return info, ac.theta.detach().clone(), float(st['step']) if len(st) else 0.0, np.random.get_state()[1].copy()

    # the KL after each epoch of this run (synchronous loop, no early stop) picks a limit that fires in the middle
    kls = [run('0', 1e9, k)[0]['approx_kl'] for k in (1, 2, 3, 4)]
    limit = None
    for k in range(1, 4):  # a limit between |kl| of epochs k-1 and k, well away from both
        lo, hi = max(kls[:k]), kls[k]
        if hi > 0 and hi > 3 * max(lo, 1e-9):
            limit = (max(lo, 0.0) * hi)**0.5 if lo > 0 else hi / 2
            expect = k
            break
    assert limit is not None, kls
    for target in (limit / 1.5, 1e9):
        i0, t0, s0, r0 = run('0', target)
        i1, t1, s1, r1 = run('1', target)
        assert i0['num_opt_steps'] == i1['num_opt_steps'] and s0 == s1
        if target < 1e8:
            assert i0['num_opt_steps'] == expect, (i0['num_opt_steps'], expect, kls)
        assert np.array_equal(r0, r1)
        # (up to six Adam steps: the run-to-run noise of the float atomics, which Adam turns into O(lr) differences on entries
        # whose gradient is ~0, grows with the number of steps; two steps hold 2e-5 in the tests above)
        assert (t0 - t1).abs().max().item() <= 1e-4 * t0.abs().max().item()
        for k in ppo.KEYS + ('grad_norm', ):
            assert abs(i0[k] - i1[k]) <= 1e-5 * max(1.0, abs(i0[k])), k


@pytest.mark.parametrize('agent', ['covariant', 'internal'])
def test_pickled_agent_steps_on_caches_of_its_own(built_lib, agent):
    """a whole-module pickle taken after an epoch-cached step carries none of the agent's caches: the copy allocates its own
    workspace and its step -- stream launches, against the original's graph launch -- gives the same six statistics bit for
    bit, as graph and stream steps of ONE agent do (test_graph_step_equals_stream_launches, here and in test_gpu_internal.py)"""
    import pickle
    from molgym_amd.spaces import ActionSpace, ObservationSpace
    from molgym_amd.synthetic import CONFIGS, MODEL_DEFAULTS, make_batch_internal
    cfg, canvas = CONFIGS['cfg2'], 5
    spaces = (ObservationSpace(canvas, cfg['zs']), ActionSpace(cfg['zs']))
    torch.manual_seed(41)
    if agent == 'covariant':
        from molgym_amd.agents.covariant import CovariantAC
        ac = CovariantAC(*spaces, bag_scale=cfg['bag_scale'], beta=cfg['beta'], device='cuda:0', **MODEL_DEFAULTS)
        d = make_batch(4, canvas, cfg['zs'], seed=90)
    else:
        from molgym_amd.agents.internal import SchNetAC
        ac = SchNetAC(*spaces, MODEL_DEFAULTS['min_max_distance'], MODEL_DEFAULTS['network_width'], device='cuda:0')
        d = make_batch_internal(4, canvas, cfg['zs'], seed=90)
    stats = ac.ppo_minibatch(ac.prepare_batch(d['obs'], d['act'], d['logp'], d['adv'], d['ret']), 0.2, 0.5, 0.01, epoch_cache=True)
    blob = pickle.dumps(ac)
    assert ac._ws_cache[0] is ac._last_ws and ac._ws_epoch[0]['weights']  # (taking the pickle left the original's caches alone)
    other = pickle.loads(blob)
    assert other._ws_cache == {} and other._ws_epoch == {} and other._last_ws is None and other._last_out is None
    other.invalidate_weights()
    batch = other.prepare_batch(d['obs'], d['act'], d['logp'], d['adv'], d['ret'])
    again = other.ppo_minibatch(batch, 0.2, 0.5, 0.01, graph=False, epoch_cache=True)
    torch.cuda.synchronize()
    print(f'\n{agent}: original {stats.tolist()}\n{agent}: copy     {again.tolist()}')
    assert not other.last_step_used_graph
    assert torch.isfinite(stats).all() and torch.equal(stats, again)
    assert other._ws_cache[0] is not ac._ws_cache[0] and other._ws_cache[0].data_ptr() != ac._ws_cache[0].data_ptr()
    assert torch.equal(other.theta, ac.theta) and torch.isfinite(other.theta.grad).all()


def test_minibatches_in_flight_accumulate_like_sequential(built_lib):
    """three mini-batches on three HIP streams (own workspaces, atomic accumulation) == the sequential sum"""
    ac, ref, cfg = make_pair('cfg2', seed=23)
    batches = []
    for k in range(3):
        d = make_batch(20 + 5 * k, cfg['canvas_size'], cfg['zs'], seed=30 + k)
        batches.append(ac.prepare_batch(d['obs'], d['act'], d['logp'], d['adv'], d['ret']))
    ac.theta.grad = torch.zeros_like(ac.theta)
    seq_stats = [ac.ppo_minibatch(b, 0.2, 0.5, 0.01).clone() for b in batches]
    torch.cuda.synchronize()
    g_seq = ac.theta.grad.clone()
    ac.theta.grad.zero_()
    streams = [torch.cuda.Stream() for _ in range(3)]
    par_stats = []
    for k, b in enumerate(batches):
        streams[k].wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(streams[k]):
            par_stats.append(ac.ppo_minibatch(b, 0.2, 0.5, 0.01, slot=k))
    for st in streams:
        torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    scale = g_seq.abs().max().item()
    assert (ac.theta.grad - g_seq).abs().max().item() < 1e-5 * scale
    for a, b in zip(seq_stats, par_stats):
        assert torch.allclose(a, b, rtol=1e-9, atol=1e-12)


def test_buffer_get_data_on_device_equals_host(built_lib):
    """DynamicPPOBuffer.get_data(device=...) (mg_gae over all paths + mg_adv_normalize) == the reference's host form"""
    from molgym_amd.buffer import PPOBufferContainer
    rng = np.random.default_rng(0)
    cont = PPOBufferContainer(size=5, gamma=0.99, lam=0.97)
    d = make_batch(5, 7, [0, 9, 16], seed=0)
    for t in range(9):
        terminals = rng.random(5) < 0.3
        cont.store(d['obs'], d['act'], rng.normal(size=5), d['obs'], terminals, rng.normal(size=5),
                   rng.normal(-4, 1, size=5))
    cont.finish_paths(rng.normal(size=5))
    buf = cont.merge()
    host, dev = buf.get_data(), buf.get_data(device='cuda:0')
    assert dev['adv'].dtype == torch.float64 and dev['adv'].is_cuda
    for k in ('adv', 'ret', 'logp'):
        np.testing.assert_allclose(dev[k].cpu().numpy(), host[k], rtol=1e-11, atol=1e-13)
    assert dev['obs'] is host['obs'] and np.array_equal(dev['act'], host['act'])


def test_train_reports_the_reference_gradient_norm_and_clips(built_lib):
    """train() takes norm / clip through mg_grad_norm_clip on the flat gradient: the reported norm is
    util.compute_gradient_norm of the accumulated gradient, the step equals clip_grad_norm_ + optimizer step"""
    from molgym_amd import ppo
    ac, ref, cfg = make_pair('cfg2', seed=31)
    data = make_batch(24, cfg['canvas_size'], cfg['zs'], seed=12)
    before = ac.theta.detach().clone()
    batch = ac.prepare_batch(data['obs'], data['act'], data['logp'], data['adv'], data['ret'])
    ac.theta.grad = torch.zeros_like(ac.theta)
    ac.ppo_minibatch(batch, 0.2, 0.5, 0.01)
    g = ac.theta.grad.clone()
    want_norm = g.norm().item()
    p = torch.nn.Parameter(before.clone())
    p.grad = g.clone()
    torch.nn.utils.clip_grad_norm_([p], 0.5)
    opt_ref = torch.optim.SGD([p], lr=0.1)  # linear in the gradient (Adam's first step is g / |g|: noise where g ~ 0)
    opt_ref.step()
    ac.theta.grad = None
    infos = ppo.train(ac, torch.optim.SGD(ac.parameters(), lr=0.1), data, mini_batch_size=24, clip_ratio=0.2,
                      target_kl=1e9, vf_coef=0.5, entropy_coef=0.01, gradient_clip=0.5, max_num_steps=1)
    assert abs(infos['grad_norm'] - want_norm) < 1e-4 * want_norm and want_norm > 0.5
    assert (ac.theta.detach() - p.detach()).abs().max().item() < 1e-6


def test_gather_rows_equals_index_select(built_lib):
    """mg_gather_rows (one launch for all the tensors of a mini-batch) against torch.index_select, mixed dtypes / widths,
    repeated and unsorted indices, and the empty selection"""
    g = torch.Generator().manual_seed(0)
    n = 1000
    ts = (torch.randn(n, 7, 3, generator=g).cuda(), torch.randint(0, 17, (n, 7), generator=g, dtype=torch.int32).cuda(),
          torch.randn(n, 3, generator=g).cuda(), torch.randn(n, 6, generator=g).cuda(),
          torch.randn(n, generator=g, dtype=torch.float64).cuda(), torch.randn(n, generator=g, dtype=torch.float64).cuda(),
          torch.randn(n, generator=g, dtype=torch.float64).cuda())
    for B in (0, 1, 140, 999):
        idx = torch.randint(0, n, (B, ), generator=g).cuda()
        got = _lib.gather_rows(ts, idx, S())
        for a, t in zip(got, ts):
            want = t.index_select(0, idx)
            assert a.dtype == t.dtype and a.shape == want.shape and a.is_contiguous()
            assert torch.equal(a, want)


@pytest.mark.parametrize('amsgrad,wd,maximize', [(True, 0.0, False), (False, 0.0, False), (True, 1e-2, False), (False, 0.0, True)])
def test_adam_step_kernel_equals_torch_adam(built_lib, amsgrad, wd, maximize):
    """mg_adam_step (through FlatThetaAgent.adam_step) against torch.optim.Adam itself over several updates: parameters and
    every state tensor, and the optimizer's own state_dict stays interchangeable (a torch step after ours continues it)."""
    ac, _, _ = make_pair('cfg2', seed=5)
    ref = torch.nn.Parameter(ac.theta.detach().clone())
    kw = dict(lr=3e-4, amsgrad=amsgrad, weight_decay=wd, maximize=maximize)
    ours, theirs = torch.optim.Adam(ac.parameters(), **kw), torch.optim.Adam([ref], **kw)
    g = torch.Generator().manual_seed(1)
    for it in range(6):
        grad = (torch.randn(ac.theta.numel(), generator=g) * (10.0 ** float(torch.randint(-3, 2, (1, ), generator=g)))).cuda()
        ac.theta.grad, ref.grad = grad.clone(), grad.clone()
        if it < 5:
            assert ac.adam_step(ours) is True
        else:
            ours.step()  # torch continues from the state our launches left
        theirs.step()
        so, st = ours.state[ac.theta], theirs.state[ref]
        assert float(so['step']) == float(st['step']) == it + 1
        for k in ('exp_avg', 'exp_avg_sq') + (('max_exp_avg_sq', ) if amsgrad else ()):
            torch.testing.assert_close(so[k], st[k], rtol=2e-6, atol=1e-12)
        torch.testing.assert_close(ac.theta.detach(), ref.detach(), rtol=1e-6, atol=1e-9)
    assert ac.adam_step(torch.optim.SGD(ac.parameters(), lr=0.1)) is False  # anything else is left to torch
