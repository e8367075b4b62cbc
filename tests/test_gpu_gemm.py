"""Every kernel form of the grouped GEMM dispatchers (csrc/gemm_dispatch.inc: launch_gemm, launch_dw) against a float64 reference.

The dispatchers choose among some seventy kernel instantiations (fourteen forms) of csrc/gemm.inc by row count, alignment, reduction length, output
width and epilogue flags; the model only reaches them at the shapes it happens to produce.  Here they are called directly
(mg_test_gemm / mg_test_gemm_dw, include/molgym_hip.h) over a sweep derived from the dispatchers' own conditions
(tests/gemm_ref.py::blocks), each branch at its natural size and at its edges, and compared per element with float64
torch.matmul on the CPU under a DERIVED bound (gemm_ref.reference_gemm / reference_dw).  Every output sits between guard rows
and has sentinel pad columns that must come back bit-identical.  forms_out says which forms a call launched;
test_every_reachable_form_ran pins the set the whole sweep reaches.

The switches of the dispatchers are read once per process: the VALU fallbacks and the same forms at other geometry (several row
tiles per cols_ws workgroup, the 16-byte weight-gradient form at small row counts) run this same file in child interpreters (tests/test_gpu_parity_full.py: _FORCED['gemm_valu'], ['gemm_alt']); gemm_ref.PROFILES has their environments and
gemm_ref.REACHABLE the expected form set of each.

Regression recorded here: the straight-line path of k_gemm_mfma_cols_ws dropped the partial last column quad when N % 4 != 0
(R = 20, N = 222, ldy = 224, plain: the last two columns kept their previous contents); such widths now take the guarded loop."""
import ctypes as C
import os

import pytest
import torch

from tests import gemm_ref as gr

pytestmark = pytest.mark.gpu

_BLOCKS = gr.blocks()
_RESULTS = {}   # block -> (OR of the forms_out masks, failures)


def _profile():
    for name, env in gr.PROFILES.items():
        if env and all(os.environ.get(k) == v for k, v in env.items()):
            return name
    return 'default'


def _run_gemm(lib, case, planned=None):
    """(rc, forms_out, failures); `planned` (a list) also receives the forms the planner alone gives for the same descriptors under
    the process's switches"""
    ops = gr.build_gemm(case)
    keep = []
    arr, ys = gr.gemm_groups(ops, lambda t: keep.append(t.cuda()) or keep[-1])
    mask, plan = C.c_uint64(0), C.c_uint64(0)
    lib.mg_test_gemm_plan(arr, len(ops), None, C.byref(plan), None)
    rc = lib.mg_test_gemm(arr, len(ops), C.byref(mask), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    if planned is not None:
        planned.append(plan.value)
    if rc != 0:
        return rc, 0, []
    return 0, mask.value, gr.check_gemm(ops, [y.cpu() for y in ys])


def _run_dw(lib, case, planned=None):
    ops = gr.build_dw(case)
    keep = []
    arr, ws, bs = gr.dw_groups(ops, lambda t: keep.append(t.cuda()) or keep[-1])
    mask, plan = C.c_uint64(0), C.c_uint64(0)
    lib.mg_test_gemm_dw_plan(arr, len(ops), None, C.byref(plan), None)
    rc = lib.mg_test_gemm_dw(arr, len(ops), C.byref(mask), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    if planned is not None:
        planned.append(plan.value)
    if rc != 0:
        return rc, 0, []
    return 0, mask.value, gr.check_dw(ops, [w.cpu() for w in ws], [b.cpu() if b is not None else None for b in bs])


def _run_block(lib, block):
    from molgym_amd import _lib
    if block in _RESULTS:
        return _RESULTS[block]
    profile = _profile()
    total, fails = 0, []
    for case in _BLOCKS[block]:
        planned = []
        rc, mask, bad = (_run_gemm if case.kind == 'gemm' else _run_dw)(lib, case, planned)
        if profile in case.einval_in:
            if rc != -1:   # MG_EINVAL
                fails.append(f'{case.label()}: expected MG_EINVAL under {profile}, got {rc}')
            continue
        if rc != 0:
            fails.append(f'{case.label()}: error {rc}: {lib.mg_last_error().decode()}')
            continue
        total |= mask
        if planned[0] != mask:
            fails.append(f'{case.label()}: launched {sorted(_lib.gemm_form_names(mask))}, the planner alone says {sorted(_lib.gemm_form_names(planned[0]))}')
        fails += [f'{case.label()} [{", ".join(sorted(_lib.gemm_form_names(mask)))}]: {f}' for f in bad]
        if profile == 'default' and case.forms is not None and _lib.gemm_form_names(mask) != set(case.forms):
            fails.append(f'{case.label()}: launched {sorted(_lib.gemm_form_names(mask))}, the dispatcher conditions say {sorted(case.forms)}')
    _RESULTS[block] = (total, fails)
    return _RESULTS[block]


@pytest.mark.parametrize('block', sorted(_BLOCKS))
def test_gemm_sweep_vs_float64(built_lib, block):
    _, fails = _run_block(built_lib, block)
    assert not fails, f'{len(fails)} failures:\n' + '\n'.join(fails[:20])


def test_every_reachable_form_ran(built_lib):
    """the OR of forms_out over the whole sweep == the forms reachable under this process's switches (gemm_ref.REACHABLE)"""
    from molgym_amd import _lib
    total = 0
    for block in sorted(_BLOCKS):
        total |= _run_block(built_lib, block)[0]
    want = set(gr.REACHABLE[_profile()])
    got = _lib.gemm_form_names(total)
    assert got == want, f'profile {_profile()}: never ran {sorted(want - got)}, unexpectedly ran {sorted(got - want)}'
    assert total >> (max(_lib.GEMM_FORMS.values()) + 1) == 0 and not total & ~sum(1 << b for b in _lib.GEMM_FORMS.values())


def test_cols_ws_partial_column_quad_regression(built_lib):
    """R = 20, N = 222, ldy = 224, plain, under the default switches: k_gemm_mfma_cols_ws is the form that runs, and the last two
    columns are computed (its straight-line path used to leave them at their previous contents)"""
    from molgym_amd import _lib
    case = [c for c in _BLOCKS['cols_misc'] if c.name.startswith('cols_ws N % 4')][0]
    rc, mask, bad = _run_gemm(built_lib, case)
    assert rc == 0 and not bad, bad
    assert _profile() != 'default' or _lib.gemm_form_names(mask) == {'cols_ws'}   # (the child profiles deselect this test)
