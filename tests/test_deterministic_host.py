"""The deterministic-mode switch on the host (no GPU): default, setter, environment, workspace size."""
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _child(code, **env):
    e = dict(os.environ)
    e.pop('MG_DETERMINISTIC', None)
    e.update(env)
    return subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)


def test_switch_defaults_to_off_and_the_setter_returns_the_previous_value(built_lib):
    """in a fresh interpreter without MG_DETERMINISTIC (this one may have been started with it)"""
    r = _child('import molgym_amd as m\n'
               'assert m.is_deterministic() is False\n'
               'assert m.set_deterministic(True) is False and m.is_deterministic() is True\n'
               'assert m.set_deterministic(True) is True\n'
               'assert m.set_deterministic(False) is True and m.is_deterministic() is False\n'
               'from molgym_amd import _lib\n'
               'assert _lib.lib().mg_set_deterministic(5) == 0 and _lib.lib().mg_get_deterministic() == 1\n'
               'print("ok")')
    assert r.returncode == 0 and r.stdout.strip() == 'ok', r.stderr


def test_environment_turns_it_on(built_lib):
    code = 'import molgym_amd as m\nprint(int(m.is_deterministic()))'
    for value, want in (('1', '1'), ('0', '0'), ('', '0')):
        r = _child(code, MG_DETERMINISTIC=value)
        assert r.returncode == 0 and r.stdout.strip() == want, (value, r.stdout, r.stderr)


def test_workspace_grows_only_while_the_switch_is_on(built_lib):
    import molgym_amd
    from molgym_amd import _lib
    prev = molgym_amd.is_deterministic()
    try:
        sizes = {}
        for width, canvas, B, TA in ((128, 7, 33, 150), (64, 7, 20, 90), (128, 20, 9, 120)):
            cfg = _lib.IntCfg()
            cfg.B, cfg.N, cfg.Z, cfg.W = B, canvas, 3, width
            for i, z in enumerate((0, 9, 16)):
                cfg.zs[i] = z
            cfg.TA, cfg.MA, cfg.ME = TA, 3 * TA + 2 * B, 3 * TA * canvas
            cfg.min_distance, cfg.max_distance = 0.8, 1.8
            for on in (False, True, False):
                molgym_amd.set_deterministic(on)
                n = C.c_size_t(0)
                _lib.check(built_lib.mg_int_workspace_bytes(C.byref(cfg), C.byref(n)))
                sizes.setdefault((width, canvas), []).append(n.value)
                off, cnt = C.c_int64(), C.c_int64()
                _lib.check(built_lib.mg_int_workspace_lookup(C.byref(cfg), b'd_v', C.byref(off), C.byref(cnt)))
                sizes.setdefault((width, canvas, 'd_v'), []).append(off.value)
        for key, v in sizes.items():
            if len(key) == 3:
                assert v[0] == v[1] == v[2], (key, v)      # nothing else moves
            else:
                assert v[0] == v[2] and v[1] > v[0], (key, v)  # off: unchanged; on: the ordered form's scratch behind it
    finally:
        molgym_amd.set_deterministic(prev)
