"""The len(zs) limit of the C header and of the Python binding are one number, and both cfg structs hold that many atomic
numbers (no GPU needed)."""
import ctypes as C
import os
import re

from molgym_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, 'include', 'molgym_hip.h')).read()


def test_binding_mirrors_the_header_zs_limit():
    m = re.search(r'^#define MG_MAX_Z (\d+)', _header(), re.M)
    assert m, 'MG_MAX_Z missing from include/molgym_hip.h'
    assert _lib.MG_MAX_Z == int(m.group(1)) == 16
    m = re.search(r'^#define MG_MAX_ZCE (\d+)', _header(), re.M)
    assert m, 'MG_MAX_ZCE missing from include/molgym_hip.h'
    assert _lib.MG_MAX_ZCE == int(m.group(1)) == 64


def test_cfg_structs_hold_sixteen_atomic_numbers():
    """both structs are int32 / float fields only (no padding): 32 bytes more than with an 8-entry zs"""
    for cls in (_lib.CovCfg, _lib.IntCfg):
        fields = dict((f[0], f[1]) for f in cls._fields_)
        assert C.sizeof(fields['zs']) == 16 * 4, cls.__name__
        with_8 = sum(C.sizeof(t) for n, t in cls._fields_ if n != 'zs') + 8 * 4
        assert C.sizeof(cls) == with_8 + 32, (cls.__name__, C.sizeof(cls))
    # the header declares both arrays by the macro
    assert len(re.findall(r'int32_t zs\[MG_MAX_Z\];', _header())) == 2
