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


def _cfg(_lib, zs, canvas, B, TA, TE, W=128, G=3):
    cfg = _lib.CovCfg()
    cfg.B, cfg.N, cfg.Z, cfg.W, cfg.G = B, canvas, len(zs), W, G
    for i, z in enumerate(zs):
        cfg.zs[i] = z
    cfg.TA, cfg.TE = TA, TE
    cfg.has_beta, cfg.beta, cfg.bag_scale = 1, -10.0, 5.0
    cfg.min_distance, cfg.max_distance = 0.8, 1.8
    return cfg


def test_workspace_grows_only_while_the_covariant_switch_is_on(built_lib):
    import molgym_amd
    from molgym_amd import _lib
    prev = (molgym_amd.is_deterministic(), molgym_amd.is_deterministic_covariant())
    try:
        for zs, canvas, B, TA, TE in (((0, 9, 16), 7, 33, 120, 600), ((0, 1, 6, 7, 8), 20, 3, 56, 1050), ((0, 1, 6, 7, 8), 40, 64, 2000, 70000)):
            cfg = _cfg(_lib, zs, canvas, B, TA, TE)
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


def test_scratch_regions_have_names_while_the_switch_is_on(built_lib):
    """mg_cov_workspace_lookup answers for ord_cg, ord_phi and ord_dw (offset and length in floats, as for every other entry) while
    mg_cov_set_ordered is on: disjoint, 256-byte aligned, behind the last ordinary entry and inside mg_cov_workspace_bytes; with
    the switch off they get the error of an unknown name and the reported size is what it was"""
    import molgym_amd
    from molgym_amd import _lib
    prev = (molgym_amd.is_deterministic(), molgym_amd.is_deterministic_covariant())
    ordinary = (b'err', b'dwexp', b'd_parts')   # (d_parts: the last entry of the arena)
    regions = (b'ord_cg', b'ord_phi', b'ord_dw')

    def lookup(cfg, name):
        off, cnt = C.c_int64(-1), C.c_int64(-1)
        rc = built_lib.mg_cov_workspace_lookup(C.byref(cfg), name, C.byref(off), C.byref(cnt))
        return rc, off.value, cnt.value

    def size(cfg):
        n = C.c_size_t(0)
        _lib.check(built_lib.mg_cov_workspace_bytes(C.byref(cfg), C.byref(n)))
        return n.value

    try:
        for args in (((0, 9, 16), 7, 33, 120, 600), ((0, 9, 16), 8, 1, 8, 64), ((0, 9, 16), 8, 2, 9, 65), ((0, 9, 16), 7, 260, 1820, 12740, 128, 8),
                     ((0, 1, 6, 7, 8), 20, 41, 820, 16400), ((0, 1, 6, 7, 8), 65, 3, 129, 8321), ((0, 1, 6, 7, 8), 40, 64, 2000, 70000, 256)):
            cfg = _cfg(_lib, *args)
            molgym_amd.set_deterministic(False)
            off_size = size(cfg)
            rc_unknown = lookup(cfg, b'no_such_entry')[0]
            assert rc_unknown != 0
            for name in regions:
                assert lookup(cfg, name)[0] == rc_unknown, name
            molgym_amd.set_deterministic(True, covariant=True)
            on_size = size(cfg)
            assert lookup(cfg, b'no_such_entry')[0] == rc_unknown
            last = 0
            for name in ordinary:
                rc, off, cnt = lookup(cfg, name)
                assert rc == 0
                last = max(last, 4 * (off + cnt))
            spans = []
            for name in regions:
                rc, off, cnt = lookup(cfg, name)
                assert rc == 0 and cnt > 0, (name, rc, off, cnt)
                spans.append((4 * off, 4 * (off + cnt)))
            assert all(b0 % 256 == 0 for b0, _ in spans), spans
            assert spans[0][0] >= last, (spans, last)                                               # behind the ordinary workspace
            assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), spans                       # disjoint, in this order
            assert spans[-1][1] <= on_size, (spans, on_size)
            molgym_amd.set_deterministic(False)
            assert size(cfg) == off_size and lookup(cfg, b'ord_cg')[0] == rc_unknown
    finally:
        molgym_amd.set_deterministic(prev[0], covariant=prev[1])
