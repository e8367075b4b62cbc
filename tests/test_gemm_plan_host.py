"""The planners of the grouped GEMM dispatchers (csrc/gemm_dispatch.inc: plan_gemm, plan_gemm_dw) over the whole sweep, without a GPU.

mg_test_gemm_plan / mg_test_gemm_dw_plan run the translation, the splits and the planners of mg_test_gemm / mg_test_gemm_dw and
count the launches instead of issuing them; the switches come as a string on top of the defaults, so the three profiles of
gemm_ref.PROFILES are planned in this one process.  The assertions are those tests/test_gpu_gemm.py makes with kernels -- per-case
forms under the default switches, MG_EINVAL where a profile refuses a call, the OR over the sweep against gemm_ref.REACHABLE -- and
their expected values were validated there, on the GPU, against the dispatcher as it was before planning and launching were
separated: they are the reference here.  Descriptors come from the same builders with CPU buffers as "device" pointers: the
planners look at alignment only and nothing dereferences them."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from tests import gemm_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_BLOCKS = gr.blocks()
_PLANS = {}   # (block, index of the case) -> {profile: (rc, forms mask, launches)}


def _switches(profile):
    return ' '.join(f'{k}={v}' for k, v in gr.PROFILES[profile].items()).encode()


def _plan(lib, case, switches_list):
    """[(rc, mask, launches)] of one case, one entry per switches string (None: the process's table); descriptors built once"""
    if case.kind == 'gemm':
        ops = gr.build_gemm(case, fill=False)
        arr, fn = gr.gemm_groups(ops)[0], lib.mg_test_gemm_plan
    else:
        ops = gr.build_dw(case, fill=False)
        arr, fn = gr.dw_groups(ops)[0], lib.mg_test_gemm_dw_plan
    out = []
    for sw in switches_list:
        mask, n = C.c_uint64(0), C.c_int32(0)
        rc = fn(arr, len(ops), sw, C.byref(mask), C.byref(n))
        out.append((rc, mask.value, n.value))
    return out


def _plans(lib):
    if not _PLANS:
        strings = [_switches(p) for p in gr.PROFILES]
        for block, cases in _BLOCKS.items():
            for i, case in enumerate(cases):
                _PLANS[block, i] = dict(zip(gr.PROFILES, _plan(lib, case, strings)))
    return _PLANS


@pytest.mark.parametrize('profile', list(gr.PROFILES))
def test_planned_forms_of_the_sweep(built_lib, profile):
    from molgym_amd import _lib
    plans, total, fails = _plans(built_lib), 0, []
    for block, cases in _BLOCKS.items():
        for i, case in enumerate(cases):
            rc, mask, launches = plans[block, i][profile]
            if profile in case.einval_in:
                if rc != -1:   # MG_EINVAL
                    fails.append(f'{case.label()}: expected MG_EINVAL under {profile}, got {rc}')
                continue
            if rc != 0:
                fails.append(f'{case.label()}: error {rc}: {built_lib.mg_last_error().decode()}')
                continue
            total |= mask
            names = _lib.gemm_form_names(mask)
            if not 1 <= len(names) <= launches:   # every launch has one form, and a non-empty call launches
                fails.append(f'{case.label()}: {launches} launches for the forms {sorted(names)}')
            if profile == 'default' and case.forms is not None and names != set(case.forms):
                fails.append(f'{case.label()}: planned {sorted(names)}, the dispatcher conditions say {sorted(case.forms)}')
    assert not fails, f'{len(fails)} failures:\n' + '\n'.join(fails[:20])
    want, got = set(gr.REACHABLE[profile]), _lib.gemm_form_names(total)
    assert got == want, f'profile {profile}: never planned {sorted(want - got)}, unexpectedly planned {sorted(got - want)}'
    assert not total & ~sum(1 << b for b in _lib.GEMM_FORMS.values())


def test_launch_counts_of_the_splits(built_lib):
    """more than GEMM_MAXG = 16 groups: two launches; mixed column tiles: one per group; weight-gradient classes: one per run, and
    more than DW_MAXG = 64 groups of one class: two; an empty group launches nothing"""
    plans = _plans(built_lib)
    groups, dw = _BLOCKS['groups'], _BLOCKS['dw_misc']
    assert len(groups[1].groups) == 19 and plans['groups', 1]['default'][2] == 2
    assert plans['groups', 6]['default'][2] == 3 and plans['groups', 0]['default'][2] == 1
    assert plans['groups', 3]['default'][2] == 1
    i70 = [i for i, c in enumerate(dw) if len(c.groups) == 70][0]
    assert plans['dw_misc', i70]['default'][2] == 2
    i7 = [i for i, c in enumerate(dw) if len(c.groups) == 7][0]   # classes 1, 1 | 3 | 2 | VALU 8 | VALU 32 | 1: six runs
    assert plans['dw_misc', i7]['default'][2] == 6


def test_unknown_switch_is_refused(built_lib):
    case = _BLOCKS['groups'][0]
    for text in (b'MG_NO_SUCH_SWITCH=1', b'MG_MFMA=0 MG_MFMA_ROWS64=1', b'MG_MFMA', b'MG_MFM=0',
                 b'MG_GEMM_RT=2', b'MG_DW4_KT=2', b'MG_ROWS64_RT2=0'):   # (the last three: switches of removed forms)
        (rc, mask, launches), = _plan(built_lib, case, [text])
        assert rc == -1 and mask == 0 and launches == 0, (text, rc, mask, launches)
        assert b'switch' in built_lib.mg_last_error()
    (rc, mask, launches), = _plan(built_lib, case, [b'  MG_MFMA=1   MG_GEMM_W16=1 '])
    assert rc == 0 and launches == 1


_CHILD = '''
import ctypes as C, json, sys
sys.path.insert(0, %r)
from tests import gemm_ref as gr
from tests.test_gemm_plan_host import _plan
from molgym_amd import _lib
blocks = gr.blocks()
out = [[_plan(_lib.lib(), blocks[b][i], [None])[0] for b, i in %r]]
print(json.dumps(out))
'''


def test_environment_and_string_agree(built_lib):
    """a child interpreter started with the `valu` environment and NULL switches plans what this process plans with the string"""
    import json
    picks = [('groups', 0), ('rows_140_R56', 4), ('cols_misc', 0), ('rows_lds', 0), ('dw_misc', 0), ('dw_misc', 8),
             ('dw_misc', [i for i, c in enumerate(_BLOCKS['dw_misc']) if c.einval_in][0])]
    env = dict(os.environ, **gr.PROFILES['valu'])
    r = subprocess.run([sys.executable, '-c', _CHILD % (ROOT, picks)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    child = [tuple(v) for v in json.loads(r.stdout.strip().splitlines()[-1])[0]]
    here = [_plans(built_lib)[b, i]['valu'] for b, i in picks]
    assert child == here, (child, here)
    assert here != [_plans(built_lib)[b, i]['default'] for b, i in picks]   # (the picks do tell the profiles apart)
