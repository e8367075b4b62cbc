"""CovariantAC's ordered-mode switch on the host (no GPU kernels): default, setter, environment, the two-switch semantics of
molgym_amd.set_deterministic, workspace size and offsets."""
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _child(code, **env):
    e = dict(os.environ)
    e.pop('MG_DETERMINISTIC', None)
    e.pop('MG_COV_ORDERED', None)
    e.update(env)
    return subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)


def test_switch_defaults_to_off_and_is_normalised(built_lib):
    r = _child('import molgym_amd as m\n'
               'from molgym_amd import _lib\n'
               'L = _lib.lib()\n'
               'assert m.is_deterministic_covariant() is False and L.mg_cov_get_ordered() == 0\n'
               'assert L.mg_cov_set_ordered(5) == 0 and L.mg_cov_get_ordered() == 1\n'
               'assert L.mg_cov_set_ordered(0) == 1 and L.mg_cov_get_ordered() == 0\n'
               'assert m.is_deterministic() is False\n'  # the first switch is another word
               'print("ok")')
    assert r.returncode == 0 and r.stdout.strip() == 'ok', r.stderr


def test_environment_turns_it_on(built_lib):
    code = 'import molgym_amd as m\nprint(int(m.is_deterministic_covariant()), int(m.is_deterministic()))'
    for value, want in (('1', '1 0'), ('0', '0 0'), ('', '0 0')):
        r = _child(code, MG_COV_ORDERED=value)
        assert r.returncode == 0 and r.stdout.strip() == want, (value, r.stdout, r.stderr)


def test_python_semantics_of_the_two_switches(built_lib):
    r = _child('import molgym_amd as m\n'
               'st = lambda: (m.is_deterministic(), m.is_deterministic_covariant())\n'
               'assert st() == (False, False)\n'
               'assert m.set_deterministic(True, covariant=True) is False and st() == (True, True)\n'
               'assert m.set_deterministic(True) is True and st() == (True, False)\n'      # without the keyword: second switch off
               'assert m.set_deterministic(True, covariant=True) is True and st() == (True, True)\n'
               'assert m.set_deterministic(False) is True and st() == (False, False)\n'
               'assert m.set_deterministic(False, covariant=True) is False and st() == (False, False)\n'  # off is off
               'assert m.set_deterministic(True, True) is False and st() == (True, True)\n'
               'print("ok")')
    assert r.returncode == 0 and r.stdout.strip() == 'ok', r.stderr


def test_workspace_grows_only_while_the_covariant_switch_is_on(built_lib):
    import molgym_amd
    from molgym_amd import _lib
    prev = (molgym_amd.is_deterministic(), molgym_amd.is_deterministic_covariant())
    try:
        for zs, canvas, B, TA, TE in (((0, 9, 16), 7, 33, 120, 600), ((0, 1, 6, 7, 8), 20, 3, 56, 1050), ((0, 1, 6, 7, 8), 40, 64, 2000, 70000)):
            cfg = _lib.CovCfg()
            cfg.B, cfg.N, cfg.Z, cfg.W, cfg.G = B, canvas, len(zs), 128, 3
            for i, z in enumerate(zs):
                cfg.zs[i] = z
            cfg.TA, cfg.TE = TA, TE
            cfg.has_beta, cfg.beta, cfg.bag_scale = 1, -10.0, 5.0
            cfg.min_distance, cfg.max_distance = 0.8, 1.8
            sizes, offs = [], []
            for det, cov in ((False, False), (True, False), (True, True), (False, False)):
                molgym_amd.set_deterministic(det, covariant=cov)
                n = C.c_size_t(0)
                _lib.check(built_lib.mg_cov_workspace_bytes(C.byref(cfg), C.byref(n)))
                sizes.append(n.value)
                pair = []
                for name in (b'err', b'dwexp'):
                    off, cnt = C.c_int64(), C.c_int64()
                    _lib.check(built_lib.mg_cov_workspace_lookup(C.byref(cfg), name, C.byref(off), C.byref(cnt)))
                    pair.append((off.value, cnt.value))
                offs.append(pair)
            assert sizes[0] == sizes[1] == sizes[3], sizes   # mg_set_deterministic alone does not change it; off again: the old value
            # on: at least the CG adjoint's scratch, 50 floats per (channel, atom or edge), behind the workspace
            assert sizes[2] >= sizes[0] + 4 * 50 * 10 * (TA + TE), sizes
            assert offs[0] == offs[1] == offs[2] == offs[3], offs
    finally:
        molgym_amd.set_deterministic(prev[0], covariant=prev[1])
