"""The GEMM comparator of tests/gemm_ref.py, proven on the CPU (no GPU, no library): with a float32 torch.matmul + float32
epilogue as the "kernel" it accepts the honest result of EVERY case of the sweep tests/test_gpu_gemm.py runs -- so "the
reference's own error stays within the bound" is a checked statement, not a hope -- and it rejects each of six subtle defects
of the kind a kernel could have."""
import pytest
import torch

from tests import gemm_ref as gr
from tests.gemm_ref import Case, D, G

_BLOCKS = gr.blocks()


def _honest(case):
    if case.kind == 'gemm':
        ops = gr.build_gemm(case)
        return gr.check_gemm(ops, [gr.float32_gemm(o) for o in ops])
    ops = gr.build_dw(case)
    outs = [gr.float32_dw(o) for o in ops]
    return gr.check_dw(ops, [w for w, _ in outs], [b for _, b in outs])


@pytest.mark.parametrize('block', sorted(_BLOCKS))
def test_float32_reference_stays_within_the_bound(block):
    fails = []
    for case in _BLOCKS[block]:
        fails += [f'{case.label()}: {f}' for f in _honest(case)]
    assert not fails, '\n'.join(fails[:20])


def test_sweep_contains_what_the_issue_names():
    cases = [c for cs in _BLOCKS.values() for c in cs]
    single = {(c.groups[0].rows, c.groups[0].N, c.groups[0].R) for c in cases if c.kind == 'gemm' and len(c.groups) == 1}
    for rows in gr.ROWS:
        for N in gr.ROW_N:
            for R in gr.ROW_R:
                assert (rows, N, R) in single
    for rows in gr.COL_ROWS:
        for N in gr.COL_N:
            for R in gr.COL_R:
                for var in ('plain', 'acc', 'rowscale', 'bias', 'mask1'):
                    assert any(g.rows == rows and g.N == N and g.R == R for c in _BLOCKS[f'cols_R{R}_{var}'] for g in c.groups)
    reg = [c for c in cases if c.kind == 'gemm' and len(c.groups) == 1 and (c.groups[0].N, c.groups[0].R, c.groups[0].ldy) == (222, 20, 224)]
    assert reg and not any((reg[0].groups[0].bias, reg[0].groups[0].acc, reg[0].groups[0].rowscale, reg[0].groups[0].mask, reg[0].groups[0].resid))
    dws = {(c.groups[0].rows, c.groups[0].N, c.groups[0].K) for c in cases if c.kind == 'dw' and len(c.groups) == 1}
    for rows in gr.DW_ROWS:
        for N in gr.DW_N:
            for K in gr.DW_K:
                assert (rows, N, K) in dws
    assert any(len(c.groups) > 16 for c in cases if c.kind == 'gemm') and any(len(c.groups) > 64 for c in cases if c.kind == 'dw')
    # every form some profile can reach has a name in the binding, and every name is reachable somewhere
    from molgym_amd import _lib
    assert set().union(*[set(v) for v in gr.REACHABLE.values()]) == set(_lib.GEMM_FORMS)


# the defects, each on shapes where it applies: (name of the corruption in gemm_ref.float32_gemm, groups)
_DEFECTS = [
    ('tail_cols', G(140, 222, 20, ldy=224)),                    # (a) the last N % 4 columns left at their previous contents
    ('tail_cols', G(65, 33, 56)),
    ('drop_k', G(140, 20, 220)),                                # (b) one reduction index omitted
    ('drop_k', G(17, 128, 8, **gr._flags('all'))),
    ('bf16', G(140, 20, 56)),                                   # (c) operands rounded to bf16 before the product
    ('bf16', G(420, 48, 220, **gr._flags('all'))),
    ('tile_shift', G(65, 20, 56)),                              # (d) one 16-row tile computed from the neighbouring tile's rows
    ('tile_shift', G(140, 222, 20, bias=True, act=1)),
    ('no_acc', G(140, 20, 56, acc=True)),                       # (e) accumulate ignored
    ('no_acc', G(64, 220, 24, **gr._flags('all'))),
    ('pad_write', G(140, 20, 56)),                              # (f) a write into a pad column
    ('pad_write', G(140, 222, 20, ldy=224)),
]


@pytest.mark.parametrize('defect,group', _DEFECTS, ids=[f'{d}-{g.rows}x{g.N}x{g.R}' for d, g in _DEFECTS])
def test_comparator_rejects_subtle_defects(defect, group):
    case = Case('gemm', [group], seed=77)
    ops = gr.build_gemm(case)
    assert gr.check_gemm(ops, [gr.float32_gemm(o) for o in ops]) == []
    fails = gr.check_gemm(ops, [gr.float32_gemm(o, corrupt=defect) for o in ops])
    assert fails, defect
    if defect == 'pad_write':
        assert 'outside' in fails[0] and len(fails) == 1
    else:
        assert 'out of bound' in fails[0]


def test_comparator_rejects_weight_gradient_defects():
    case = Case('dw', [D(420, 33, 57, db=True, w0=True, ldw_pad=3)], seed=78)
    ops = gr.build_dw(case)
    w, b = gr.float32_dw(ops[0])
    assert gr.check_dw(ops, [w], [b]) == []
    o = ops[0]
    d = o['g']
    inner = lambda t: t[o['w_base']:o['w_base'] + d.N * o['ldw']].view(d.N, o['ldw'])
    # dW overwritten instead of accumulated
    w2 = w.clone()
    inner(w2)[:, :d.K] -= o['w_old']
    assert gr.check_dw(ops, [w2], [b])
    # one row of the reduction dropped
    w3 = w.clone()
    inner(w3)[:, :d.K] -= torch.outer(o['dY'][1][7, :d.N], gr._dw_x(o)[7])
    assert gr.check_dw(ops, [w3], [b])
    # db summed over one row too few
    b2 = b.clone()
    b2[o['b_base']:o['b_base'] + d.N] -= o['dY'][1][7, :d.N]
    assert gr.check_dw(ops, [w], [b2])
    # a write into the pad columns of dW, and one into the guard row in front of db
    w4 = w.clone()
    inner(w4)[3, d.K] = 0.0
    assert any('outside' in f for f in gr.check_dw(ops, [w4], [b]))
    b3 = b.clone()
    b3[o['b_base'] - 1] = 0.0
    assert any('outside' in f for f in gr.check_dw(ops, [w], [b3]))
