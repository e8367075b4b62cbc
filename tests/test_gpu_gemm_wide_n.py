"""The GEMM widths that element sets of 9..16 symbols bring to the dispatchers (csrc/state.inc), called directly.

The last atom level of CovariantAC mixes into Co = len(zs) * num_channels_per_element complex channels: a real GEMM of
N = 2 Co columns (72 .. 128 for 9 .. 16 symbols at 4 channels per element; 104 = 13 symbols has a partial last 16-column
tile), its input adjoint a GEMM of R = 2 Co (past the R <= 64 column forms: the row forms take it), and its weight gradient one
of N = 2 Co, plain and over the concatenated input.  Reference, derived bound and guard checking are those of tests/gemm_ref.py;
the operands are uploaded and the library called as in tests/test_gpu_gemm.py."""
import pytest

from tests import gemm_ref as gr
from tests.test_gpu_gemm import _run_dw, _run_gemm

pytestmark = pytest.mark.gpu

WIDE = (72, 104, 128)   # 2 * Z * CE for Z = 9, 13, 16 at CE = 4
ROWS = (40, 300)
LONG = 210              # the concatenated input of the mix (K of the forward, N of its adjoint)
# The concatenated weight gradient reads columns [0, 80) | [80, 160) | [160, K) from three matrices.  launch_dw takes such an input
# only with every segment's pitch a multiple of 4 floats (it refuses anything else with MG_EINVAL, "misaligned segment": the model's
# arena rows are), and gemm_ref.build_dw gives a segment the pitch of its width: K = 210 would leave the last one 50 floats wide.
# So this one case runs at K = 212, the nearest legal length; the plain weight gradient keeps K = 210.
LONG_CAT = 212


def _cases(x_off):
    out, seed = [], 7000 + 100 * x_off
    for rows in ROWS:
        for n in WIDE:
            groups = [
                ('gemm', gr.G(rows, n, LONG, x_off=x_off)),                        # forward mix
                ('gemm', gr.G(rows, LONG, n, x_off=x_off)),                        # its input adjoint, one segment
                ('dw', gr.D(rows, n, LONG, db=True, x_off=x_off)),                 # weight gradient, plain
                ('dw', gr.D(rows, n, LONG_CAT, cat=(80, 160), db=True, x_off=x_off)),  # ... over the concatenated input
            ]
            for kind, g in groups:
                seed += 1
                out.append(gr.Case(kind, [g], seed=seed))
    return out


@pytest.mark.parametrize('x_off', [0, 1], ids=['aligned', 'x_off1'])
def test_wide_n_forms_vs_float64(built_lib, x_off):
    """x_off = 1: X starts one float past a 16-byte boundary, so the guarded forms run"""
    fails = []
    for case in _cases(x_off):
        rc, mask, bad = (_run_gemm if case.kind == 'gemm' else _run_dw)(built_lib, case)
        if rc != 0:
            fails.append(f'{case.label()}: error {rc}: {built_lib.mg_last_error().decode()}')
        fails += [f'{case.label()}: {f}' for f in bad]
    assert not fails, f'{len(fails)} failures:\n' + '\n'.join(fails[:20])
