"""The canvas_size limit of the C header and of the Python binding are one number (no GPU needed)."""
import os
import re

from molgym_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_binding_mirrors_the_header_canvas_limit():
    text = open(os.path.join(ROOT, 'include', 'molgym_hip.h')).read()
    m = re.search(r'^#define MG_MAX_CANVAS (\d+)', text, re.M)
    assert m, 'MG_MAX_CANVAS missing from include/molgym_hip.h'
    assert _lib.MG_MAX_CANVAS == int(m.group(1)) == 255
