"""The shape seams of the default launch plan, on both sides of each comparison, against the float64 oracle -- and, from the launch
log (include/molgym_hip.h mg_launch_log_enable), WHICH form ran.  No environment switch is set anywhere in this file: every case
reaches its kernels through the shape of the mini-batch alone, as ppo.train does.

The expected kernel spellings are literals, derived by hand from the predicates of the dispatch code (default build CH = 10):

  side stream, shared DotMatrix block   TE >= 16384 each                                  (state.inc side_min_edges / sx_min_rows)
  lists_done (k_prep_lists)             one stream and B <= 256 and N <= 16, else k_lists_small in that shape (side stream on),
                                        else k_prep_counts + k_fill_lists                 (molgym_hip.hip cov_forward_impl)
  level0_fused                          lists_done and N <= 16 and TA, TE > 0 and TE < 16384                       (level0.inc)
  front_lists (k_level0_fwd<true, ..>)  level0_fused and MG_STEP_WEIGHTS_CURRENT and not sampling; NC = 8 for N <= 8, L0_MAXN
                                        above; a third argument MG_MAX_Z for Z > 8
  edge_level_fused (k_edge_fwd)         level0_fused and 4 (1701 N + 4) <= 65536 bytes of LDS, i.e. N <= 9      (edge_level.inc)
  cgm_chunked (<true> forms)            (10 TA + 3) / 4 >= 4096, i.e. TA >= 1639                                   (cg_mfma.inc)
  one stream, not fused                 k_geom_input; with the side stream: k_geom and k_input_linear
  schnet_fused                          network_width / 2 == 64 and N + 1 <= 16                                (schnet_fused.inc)
  int_heads_fused                       N <= 16 and N + Z + 6 <= 64 and 4 (768 (N + 5) + 272) <= 65536 bytes of LDS at width
                                        128 and Z <= 8 -- N <= 15: at N = 16 the layout needs 65600 bytes, so the LDS bound, not
                                        `N <= 16`, is the seam of the default width                          (int_heads_fused.inc)

The numbers are those of tests/test_gpu_large.py::test_masked_oracle_comparison_at_full_size (tests/helpers.py
masked_oracle_check): rel_err < 1e-5 on logp / ent / v of 16 named-and-drawn samples, assert_grads' defaults on every slot."""
import numpy as np
import pytest
import torch

from molgym_amd.spaces import ActionSpace, ObservationSpace
from molgym_amd.synthetic import CONFIGS, make_batch, make_batch_internal
from tests.helpers import PPO_HP, crowded, device_batch, launch_log, make_pair, masked_oracle_check, rel_err

pytestmark = pytest.mark.gpu
ZS16 = [0, 1, 5, 6, 7, 8, 9, 14, 15, 16, 17, 33, 34, 35, 52, 53]   # tests/test_gpu_wide_zs.py
L0_FALSE = 'k_level0_fwd<false, L0_MAXN>'   # the fused level 0 behind k_prep_lists, Z <= 8


def _config(monkeypatch, name, zs, canvas):
    monkeypatch.setitem(CONFIGS, name, dict(zs=list(zs), canvas_size=canvas, batch=16, bag_scale=5, beta=-10.0))
    return name


def _sizes(ac, data):
    """(B, TA, TE) as the agent's own configuration of this mini-batch holds them"""
    counts = np.array([sum(1 for label, _ in canvas if label != 0) for canvas, _ in data['obs']])
    cfg = ac._make_cfg(len(counts), counts)
    return cfg, (cfg.B, cfg.TA, cfg.TE)


def _no_list_errors(ac, cfg):
    """encoder.inc: err = 1 atoms not compacted to the front, 2 = TA / TE do not match the charges"""
    assert int(ac.workspace_view_int('err', cfg)[0]) == 0


def _ppo_log(ac, data):
    """forward AND backward of the mini-batch in one call on this thread, as stream launches: the log holds both directions"""
    batch = device_batch(ac, data)
    ac.theta.grad = None
    with launch_log() as log:
        ac.ppo_minibatch(batch, *PPO_HP, graph=False)
    torch.cuda.synchronize()
    assert torch.isfinite(ac.theta.grad).all()
    return log


# ---- TE 16383 | 16384: the side stream, the shared dot block and the fused level 0 flip together -------------------------------
@pytest.mark.parametrize('extra,sizes', [([], (68, 1031, 16383)), ([1], (69, 1032, 16384))], ids=['te16383', 'te16384'])
def test_side_stream_threshold_on_canvas_16(built_lib, monkeypatch, extra, sizes):
    """Canvas 16, B <= 256.  Below: one stream, k_prep_lists carries the list build and level 0 is the fused kernel.  At: the
    side stream prepares the weights, so the list build is k_lists_small -- its only launch site -- and the unfused level-0 and
    edge kernels, the shared DotMatrix block and the side stream all read lists in its atom_perm order."""
    counts = [16] * 63 + [15, 5, 2, 1, 0] + extra
    order = np.random.default_rng(11).permutation(len(counts))
    counts = [counts[i] for i in order]                      # (atom_perm, sorted by molecule size, is not the natural order)
    name = _config(monkeypatch, 'seam_te', CONFIGS['cfg3']['zs'], 16)
    ac, ref, _ = make_pair(name, seed=41)
    data = crowded(name, counts, seed=42)
    cfg, got = _sizes(ac, data)
    assert got == sizes
    must = [counts.index(n) for n in (0, 1, 2, 5, 15)] + [0, len(counts) - 1]
    log = masked_oracle_check(ac, ref, data, must, seed=43)
    _no_list_errors(ac, cfg)
    print(sizes, sorted(set(log.names)))
    if sizes[2] < 16384:
        assert log.ran('k_prep_lists') and log.ran(L0_FALSE)
        assert not log.ran('k_lists_small') and not log.ran('k_geom') and not log.ran('k_geom_input')
        assert not log.ran('k_edge_fwd') and log.ran('k_dot')   # (canvas 16 > 9: the edge levels stay unfused)
    else:
        assert log.ran('k_lists_small') and log.ran('k_geom') and log.ran('k_input_linear') and log.ran('k_dot0')
        assert not log.ran('k_geom_input') and not log.ran('k_level0_fwd') and not log.ran('k_edge_fwd')
        assert not log.ran('k_prep_lists') and not log.ran('k_prep_counts') and not log.ran('k_fill_lists')


# ---- B 256 | 257 and 512 | 513 on cfg2 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [256, 257, 512, 513])
def test_batch_size_thresholds_on_cfg2(built_lib, B):
    """256 | 257: the small list build with fused level 0 and edge levels against the two-kernel list build with the unfused
    chain.  512 | 513: k_heads_bwd's grid y = 3 against y = 1 (backward.inc) -- not visible in a name, covered by the numbers; the
    log holds the unfused chain on both sides."""
    ac, ref, cfg_ = make_pair('cfg2', seed=44)
    data = make_batch(B, cfg_['canvas_size'], cfg_['zs'], seed=45 + B)
    cfg, (b, TA, TE) = _sizes(ac, data)
    assert b == B and 0 < TE < 16384                     # (one stream on every side of these seams)
    must = {256: [0, 1, 255], 257: [0, 1, 255, 256], 512: [0, 511], 513: [0, 511, 512]}[B]
    log = masked_oracle_check(ac, ref, data, must, seed=46)
    _no_list_errors(ac, cfg)
    print(B, TA, TE, sorted(set(log.names)))
    assert log.ran('k_heads_fwd') and log.ran('k_catbuild_mfma') and not log.ran('k_lists_small')
    if B <= 256:
        assert log.ran('k_prep_lists') and log.ran(L0_FALSE) and log.ran('k_edge_fwd')
        assert not log.ran('k_prep_counts') and not log.ran('k_fill_lists') and not log.ran('k_dot0') and not log.ran('k_dot')
    else:
        assert log.ran('k_prep_counts') and log.ran('k_fill_lists') and log.ran('k_geom_input')
        assert log.ran('k_dot0') and log.ran('k_catbuild0') and log.ran('k_dot')
        assert not log.ran('k_level0_fwd') and not log.ran('k_edge_fwd') and not log.ran('k_prep_lists')
    both = _ppo_log(ac, data)                            # the adjoint chain follows the same predicates
    assert both.ran('k_heads_bwd')
    if B <= 256:
        assert both.ran('k_edge_level0_bwd') or both.ran('k_level0_bwd')
        assert not both.ran('k_dot0_bwd')
    else:
        assert both.ran('k_dot0_bwd') and both.ran('k_catbuild0_bwd_t<false>')
        assert not both.ran('k_level0_bwd') and not both.ran('k_edge_level0_bwd') and not both.ran('k_edge_bwd')


# ---- TA 1638 | 1639: the chunked forms of the CG product kernels -----------------------------------------------------------------
@pytest.mark.parametrize('extra,sizes', [([], (234, 1638, 11466)), ([1], (235, 1639, 11467))], ids=['ta1638', 'ta1639'])
def test_cg_chunk_threshold_on_cfg2(built_lib, extra, sizes):
    """234 full canvases of 7 are 16380 (atom, channel) items = 4095 workgroups of 4; one more atom makes 4098 >= 4096 and both
    directions of the CG product take their <true> instantiation"""
    counts = [7] * 234 + extra
    ac, ref, _ = make_pair('cfg2', seed=47)
    data = crowded('cfg2', counts, seed=48)
    cfg, got = _sizes(ac, data)
    assert got == sizes
    log = masked_oracle_check(ac, ref, data, [0, len(counts) - 1], seed=49)
    _no_list_errors(ac, cfg)
    both = _ppo_log(ac, data)
    print(sizes, sorted(set(both.names)))
    here, other = ('<true>', '<false>') if sizes[1] >= 1639 else ('<false>', '<true>')
    assert log.ran('k_catbuild_mfma' + here) and not log.ran('k_catbuild_mfma' + other)
    assert both.ran('k_catbuild_mfma' + here) and not both.ran('k_catbuild_mfma' + other)
    assert both.ran('k_catbuild_bwd_mfma' + here) and not both.ran('k_catbuild_bwd_mfma' + other)
    assert log.ran(L0_FALSE) and log.ran('k_edge_fwd')    # (B <= 256, canvas 7: still the fused chain around them)


# ---- the FRONT forms of k_level0_fwd: the first launch of every epoch-cache step after a slot's first ------------------------------
FRONT = {
    'n12_z5': (CONFIGS['cfg3']['zs'], 12, 'k_level0_fwd<true, L0_MAXN>', L0_FALSE),
    'n16_z5': (CONFIGS['cfg3']['zs'], 16, 'k_level0_fwd<true, L0_MAXN>', L0_FALSE),
    'n6_z9': (ZS16[:9], 6, 'k_level0_fwd<true, 8, MG_MAX_Z>', 'k_level0_fwd<false, L0_MAXN, MG_MAX_Z>'),
    'n12_z9': (ZS16[:9], 12, 'k_level0_fwd<true, L0_MAXN, MG_MAX_Z>', 'k_level0_fwd<false, L0_MAXN, MG_MAX_Z>'),
}
FRONT_ALL = sorted({v[2] for v in FRONT.values()} | {'k_level0_fwd<true, 8>'})


@pytest.mark.parametrize('case', sorted(FRONT))
def test_front_list_forms_at_256_samples(built_lib, monkeypatch, case):
    """B = 256 fills s_n[MG_LISTS_SMALL_B] of level0.inc; runs of empty canvases at the front, in the middle and at the end give
    the scan and the binary search of the other workgroups' descriptors repeated offsets on every side.  (i) the batch against
    the oracle; (ii) tests/test_gpu_ppo.py::test_epoch_cache_equals_per_minibatch_preparation at this shape: the SECOND
    epoch-cache step of a slot runs k_level0_fwd<true, ...> with no list or weight preparation, and equals the uncached step."""
    zs, N, front, plain = FRONT[case]
    B = 256
    rng = np.random.default_rng(50)
    counts = rng.integers(1, min(N, 8) + 1, size=B)       # (TE stays below 16384 at canvas 16: mean n^2 = 25.5)
    counts[[3, 130]] = N                                   # full canvases, each next to an empty run
    empty = [0, 1, 2, 127, 128, 129, 254, 255]
    counts[empty] = 0
    counts = [int(n) for n in counts]
    name = _config(monkeypatch, 'seam_front_' + case, zs, N)
    ac, ref, _ = make_pair(name, seed=51)
    data = crowded(name, counts, seed=52)
    cfg, (b, TA, TE) = _sizes(ac, data)
    assert b == B and 0 < TE < 16384 and N in counts
    # (i) neighbours of each empty run, an empty sample of each run, the last non-empty sample (253: a neighbour too)
    log = masked_oracle_check(ac, ref, data, [3, 126, 130, 253, 1, 128, 255], seed=53)
    _no_list_errors(ac, cfg)
    assert log.ran('k_prep_lists') and log.ran(plain) and not any(log.ran(f) for f in FRONT_ALL)
    assert log.ran('k_edge_fwd') == (N <= 9)
    # (ii)
    batch = device_batch(ac, data)
    for graph in (True, False):
        ac.theta.grad = torch.zeros_like(ac.theta)
        ac.invalidate_weights()
        ac.ppo_minibatch(batch, *PPO_HP, loss_scale=0.5, graph=graph, epoch_cache=True)
        with launch_log() as second:
            st1 = ac.ppo_minibatch(batch, *PPO_HP, loss_scale=0.5, graph=graph, epoch_cache=True).clone()
        assert ac.last_step_used_graph == graph
        o1 = ac._last_out.clone()
        ac.fold_gradients()
        torch.cuda.synchronize()
        _no_list_errors(ac, batch.cfg)
        g1 = ac.theta.grad.clone()
        ac.theta.grad = torch.zeros_like(ac.theta)
        st0 = ac.ppo_minibatch(batch, *PPO_HP, loss_scale=0.5, graph=graph, epoch_cache=False).clone()
        torch.cuda.synchronize()
        o0, g0 = ac._last_out.clone(), 2.0 * ac.theta.grad       # (the cached epoch holds the same mini-batch twice)
        print(case, 'graph' if graph else 'stream', second.names[:3], (g1 - g0).abs().max().item() / g0.abs().max().item())
        assert second.ran(front) and not any(second.ran(f) for f in FRONT_ALL if f != front)
        assert not second.ran(plain) and not second.ran('k_prep_lists') and not second.ran('k_prep_weights')
        assert not second.ran('k_lists_small') and not second.ran('k_prep_counts')
        assert torch.equal(st0, st1) and torch.equal(o0, o1)
        assert torch.isfinite(g1).all() and (g1 - g0).abs().max().item() <= 2e-5 * g0.abs().max().item()


# ---- SchNetAC N = 15 | 16 | 17 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('canvas', [15, 16, 17])
def test_schnet_canvas_thresholds(built_lib, canvas):
    """tests/test_gpu_internal.py::test_outputs_and_gradients_match_oracle at width 128, B = 9 (sample 0 empty, sample 1 full).
    15: the interactions and the heads as one launch each per direction, 16-atom layouts.  16: N + 1 = 17 molecule slots leave
    the fused interactions, and the fused heads' LDS layout (65600 bytes at width 128) leaves the 64 KB a launch gets: per-layer
    launches and grouped head GEMMs, as at 17."""
    from molgym_amd.agents.internal import SchNetAC
    from oracle.internal_ref import SchNetACRef
    zs, width, B = [0, 9, 16], 128, 9
    torch.manual_seed(0)
    ac = SchNetAC(ObservationSpace(canvas, zs), ActionSpace(zs), (0.8, 1.8), width, device='cuda:0')
    with torch.no_grad():
        g = torch.Generator().manual_seed(1)
        for name, (off, shape) in ac.slot_table.items():
            n = int(np.prod(shape))
            if name.endswith('bias'):
                ac.theta[off:off + n] = (0.1 * torch.randn(n, generator=g)).to(ac.theta)
    ref = SchNetACRef(zs, canvas, (0.8, 1.8), width).double()
    ref.load_state_dict({k: v.double().cpu() for k, v in ac.export_state_dict().items()}, strict=True)
    data = make_batch_internal(B, canvas, zs, seed=54)
    counts = [sum(1 for label, _ in c if label != 0) for c, _ in data['obs']]
    assert counts[0] == 0 and counts[1] == canvas
    g = torch.Generator().manual_seed(2)
    wl, we, wv = (torch.randn(B, generator=g, dtype=torch.float64) * s for s in (1.0, 0.3, 0.7))
    with launch_log() as log:
        out = ac.step(data['obs'], data['act'])
    (out['logp'].double() * wl.cuda() + out['ent'].double() * we.cuda() + out['v'].double() * wv.cuda()).sum().backward()
    torch.cuda.synchronize()
    exp = ref.step(data['obs'], data['act'], dtype=torch.float64)
    (exp['logp'] * wl + exp['ent'] * we + exp['v'] * wv).sum().backward()
    errs = {k: rel_err(out[k], exp[k]) for k in ('logp', 'ent', 'v')}
    print(canvas, errs, sorted(set(log.names)))
    for k, e in errs.items():
        assert e < 1e-5, (k, e)
    got, want, bad = ac.theta.grad.double().cpu(), dict(ref.named_parameters()), {}
    for name, (off, shape) in ac.slot_table.items():
        n = int(np.prod(shape))
        gw = want[name].grad
        gw = torch.zeros(n, dtype=torch.float64) if gw is None else gw.reshape(-1)
        scale = gw.abs().max().item()
        err = (got[off:off + n] - gw).abs().max().item() / max(scale, 1e-12)
        if not (err < 2e-4 or scale < 1e-10):
            bad[name] = (err, scale)
    assert not bad, bad
    batch = ac.prepare_batch(data['obs'], data['act'], data['logp'], data['adv'], data['ret'])
    ac.theta.grad = None
    with launch_log() as both:
        ac.ppo_minibatch(batch, *PPO_HP, graph=False)
    torch.cuda.synchronize()
    for lg in (log, both):
        if canvas <= 15:
            assert lg.ran('k_schnet_fwd<16>') and lg.ran('k_int_heads_fwd_pre<16>')
            assert not lg.ran('k_cfconv') and not lg.ran('k_int_inputs') and not lg.ran('k_schnet_fwd<8>')
        else:
            assert lg.ran('k_cfconv') and lg.ran('k_int_inputs')
            assert not lg.ran('k_schnet_fwd') and not lg.ran('k_int_heads_fwd_pre') and not lg.ran('k_int_heads_fwd')
    if canvas <= 15:
        assert both.ran('k_schnet_bwd<16>') and both.ran('k_int_heads_bwd_pre<16>')
    else:
        assert not both.ran('k_schnet_bwd') and not both.ran('k_int_heads_bwd_pre') and not both.ran('k_int_heads_bwd')
