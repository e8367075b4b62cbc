"""The small-batch row passes after the change of their store policy (write-through stores, the mix epilogue through a buffer
resource): what they leave in memory is what the float64 oracle computes, on the first step and on a second one.

Write-through only changes WHERE a stored line lives when the launch ends; a site that wrote through bytes a later wave of the same
launch loads, a resource sized short of an atom's last row or a line left behind by an earlier step would all show as wrong rows or
wrong gradients, so the checks are the ones of tests/test_gpu_catrows_compact.py, whose shapes and helpers are reused:
  c7    canvas 7, samples with 0, 1, 2 and 7 atoms: no item, no neighbour, one neighbour, a partial neighbour tile
  c12   canvas 12, samples with 10 and 12 atoms: a second neighbour tile, longer rows through the resource-sized stores
Builds (10, 4) and (7, 3): on the odd build K = 14 W' is no multiple of 4, the epilogue of k_edge_bwd_mix gives way to the column
GEMM, and 70 (atom, channel) items leave a partial last logical workgroup of the CG forward.

Bounds are the project's own (tests/helpers.py): a saved stage max |err| / max |want| < 1e-5, gradients assert_grads."""
import pytest
import torch

from oracle import so3
from tests.helpers import assert_grads, crowded, grad_report, oracle_backward
from tests.test_catrow_map_host import NBLK, WIDTHS, expected_map
from tests.test_gpu_catrows_compact import BUILDS, CASES, LEVELS, SHAPES, _ids, _pair_data, _run

pytestmark = pytest.mark.gpu


def _assert_rows(tag, CH, ref, d, views):
    """stored rows cat_a{k}_{l} of the levels >= 1 against the oracle's [ag | in | sq] picked through the row map"""
    with torch.no_grad():
        atoms_all, edges_all, extra = ref.cg_model(d, return_all=True)
        cg = ref.cg_model.cg.to(torch.float64)
    am = d['atom_mask']
    TA = int(am.sum())
    emap = expected_map()
    worst = 0.0
    for k in range(1, LEVELS):
        with torch.no_grad():
            reps = atoms_all[k - 1]
            ag = so3.cg_product(cg, so3.scalar_times_vec(edges_all[k], extra['sph']), reps, 4, aggregate=True)
            sq = so3.cg_product(cg, reps, reps, 4)
        for l in range(5):
            cat = torch.cat([ag[l], reps[l], sq[l]], dim=-3)[am]   # (TA, (2 nblk + 1) CH, 2l + 1, 2), channel = part * CH + c
            Ws, nm = WIDTHS[l], 2 * l + 1
            ld = (2 * CH * Ws + 31) // 32 * 32
            got = views[f'cat_a{k}_{l}'][:TA * nm * ld].view(TA, nm, ld)[:, :, :2 * CH * Ws].reshape(TA, nm, CH, Ws, 2).double()
            want = cat.reshape(TA, 2 * NBLK[l] + 1, CH, nm, 2)[:, emap[l][0]].permute(0, 3, 2, 1, 4)   # (TA, m, c, cs, 2)
            err = (got - want).abs().max().item() / max(want.abs().max().item(), 1e-30) if TA else 0.0
            print(f'{tag} cat_a{k}_{l}: max |err| / max |want| = {err:.3e}')
            worst = max(worst, err)
            assert err < 1e-5, (tag, k, l, err)
    assert TA == 0 or worst > 0.0


def _assert_gradients(tag, ac, grad, want):
    report = grad_report(grad.double(), want, ac.slot_table)
    print(f'{tag}: worst gradient slot (err / slot max)', max(v[0] for v in report.values() if v[1] >= 1e-10))
    assert bool(torch.isfinite(grad).all())
    assert_grads(report)


@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_stored_rows_vs_oracle(built_lib, case):
    build, shape = case
    run = _run(build, shape)
    _assert_rows(f'build {build} shape {shape}', build[0], run['ref'], run['d'], run['views'])


@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_every_gradient_slot_vs_oracle(built_lib, case):
    build, shape = case
    run = _run(build, shape)
    _assert_gradients(f'build {build} shape {shape}', run['ac'], run['grad'], run['want'])


@pytest.mark.parametrize('build', BUILDS, ids=lambda b: 'c%de%d' % b)
def test_second_step_on_the_same_workspace(built_lib, build):
    """the same agent and workspace, two sets of canvases of one shape one after the other: every row pass overwrites what the first
    step stored at the same addresses, and the SECOND step is held to the oracle -- a line of the first step that outlived its
    launch in some cache would be read here"""
    from oracle.covariant_ref import parse_observations
    ac, ref, cfg, first = _pair_data(build, 'c7')
    canvas, counts = SHAPES['c7']
    second = crowded(f'cfg2_canvas{canvas}', counts, 1071)
    B = len(counts)
    g = torch.Generator().manual_seed(19)
    w = tuple(torch.randn(B, generator=g, dtype=torch.float64) * s for s in (1.0, 0.3, 0.7))
    d = ccfg = rows_before = None
    for data in (first, second):
        ac.theta.grad = None
        out = ac.step(data['obs'], data['act'])
        (out['logp'].double() * w[0].cuda() + out['ent'].double() * w[1].cuda() + out['v'].double() * w[2].cuda()).sum().backward()
        torch.cuda.synchronize()
        d2 = parse_observations(data['obs'], cfg['zs'], cfg['canvas_size'], torch.float64)
        c2 = ac._make_cfg(B, d2['num_atoms'].numpy())
        if ccfg is not None:   # same shape -> same workspace
            assert (c2.B, c2.TA, c2.TE) == (ccfg.B, ccfg.TA, ccfg.TE)
            assert ac.workspace_view('cat_a1_0', c2).data_ptr() == ac.workspace_view('cat_a1_0', ccfg).data_ptr()
            assert not torch.equal(ac.workspace_view('cat_a1_0', c2).cpu(), rows_before)   # (other canvases: other rows)
        d, ccfg = d2, c2
        rows_before = ac.workspace_view('cat_a1_0', c2).detach().cpu().clone()
    views = {f'cat_a{k}_{l}': ac.workspace_view(f'cat_a{k}_{l}', ccfg).detach().cpu().clone() for k in range(1, LEVELS) for l in range(5)}
    _, want = oracle_backward(ref, second, w)
    tag = f'build {build} second step'
    _assert_rows(tag, build[0], ref, d, views)
    _assert_gradients(tag, ac, ac.theta.grad.detach().cpu(), want)
