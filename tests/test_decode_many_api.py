"""CPU: the surface of bzh_decode_many -- the header, SIGNATURES and the library agree on the four functions, the bound of the
LDS inverse BWT is a pure host number, and the Python entry points check their arguments before any context is made."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("bzh_decode_many_device", "bzh_decode_many", "bzh_decode_many_small_max", "bzh_get_decode_many_stats")


def test_header_signatures_and_library_agree(native):
    text = open(os.path.join(ROOT, "include", "bzhip.h")).read()
    declared = set(re.findall(r"BZH_API[^;(]*?\b(bzh_\w+)\s*\(", text))
    L = ctypes.CDLL(native.LIB_PATH)
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/bzhip.h"
        assert name in native.SIGNATURES, f"{name} is missing from SIGNATURES"
        assert hasattr(L, name), f"{name} is not exported"
    assert native.MISSING == []
    assert "bzh_decode_many_stats" in text and "blocks_small" in text and "ms_unbwt_small" in text
    assert len(native.SIGNATURES["bzh_decode_many_device"][1]) == 12 and len(native.SIGNATURES["bzh_decode_many"][1]) == 10


def test_small_max_is_a_host_number(native):
    """no context, no device: at least 8,192 (any input up to 6,553 bytes behind RLE1's worst 4 -> 5 expansion), at most what
    16-bit indices reach"""
    assert 8192 <= native.decode_many_small_max() <= 65536
    assert ctypes.sizeof(native.DecodeManyStats) == 56


def test_null_handles_are_refused(native):
    L = native.lib()
    st = native.DecodeManyStats()
    assert L.bzh_get_decode_many_stats(None, ctypes.byref(st)) == -1
    assert L.bzh_decode_many_device(None, None, 0, None, None, 0, None, 0, None, None, None, None) == -1
    assert L.bzh_decode_many(None, None, None, 0, None, 0, None, None, None, None) == -1


def test_python_argument_checks_come_first():
    """type and errors= checks raise before a context (and with it a device) is asked for"""
    import banzai_amd
    assert "decompress_many" in banzai_amd.__all__
    with pytest.raises(ValueError):
        banzai_amd.decompress_many([b"BZh9"], errors="ignore")
    with pytest.raises(ValueError):
        banzai_amd.decompress_many([], errors=None)
    for bad in (["text"], [b"ok", 7], [None]):
        with pytest.raises(TypeError):
            banzai_amd.decompress_many(bad)
    assert banzai_amd.decompress_many([]) == []
    assert banzai_amd.decompress_many(iter(())) == []
