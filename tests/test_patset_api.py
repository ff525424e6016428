"""CPU: the pattern set's surface without a device -- what the header declares, that the built library exports it, that the
bindings' structs have the header's sizes and fields, and what the Python layer refuses before it touches a device."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("bzh_patset_create", "bzh_patset_destroy", "bzh_patset_get_info",
         "bzh_search_patset_raw_device", "bzh_search_patset_device", "bzh_search_patset", "bzh_search_patset_range_device",
         "bzh_search_patset_range", "bzh_grep_patset_raw_device", "bzh_grep_patset_device", "bzh_grep_patset",
         "bzh_grep_patset_index_device", "bzh_grep_patset_index")


def header():
    return open(os.path.join(ROOT, "include", "bzhip.h")).read()


def test_header_declares_the_pattern_set():
    text = header()
    syms = set(re.findall(r"BZH_API[^;(]*?\b(bzh_\w+)\s*\(", text))
    for need in FUNCS:
        assert need in syms, need
    assert "typedef struct bzh_patset bzh_patset;" in text
    assert re.search(r"enum \{ BZH_PATSET_FOLD_ASCII = 1 \};", text) and re.search(r"#define BZH_PATSET_MAX_PATTERNS 65536\b", text)
    m = re.search(r"typedef struct \{([^}]*)\}\s*bzh_set_hit;", text)
    assert m, "bzh_set_hit is not declared"
    assert re.sub(r"\s+", " ", m.group(1)).strip() == "uint64_t off, record; uint32_t pattern, len;"
    m = re.search(r"typedef struct \{([^}]*)\}\s*bzh_patset_info;", text)
    assert m, "bzh_patset_info is not declared"
    body = re.sub(r"/\*.*?\*/", "", m.group(1))
    assert re.sub(r"\s+", " ", body).strip() == ("uint64_t patterns, distinct; uint32_t min_len, max_len; uint32_t states, classes; "
                                                 "uint64_t table_bytes;")
    # each twin takes its single-pattern call's arguments with (pat, plen) replaced by the set
    for twin in FUNCS[3:]:
        one = twin.replace("_patset", "")
        a = re.search(r"BZH_API int %s\(([^;]*)\);" % one, text).group(1)
        b = re.search(r"BZH_API int %s\(([^;]*)\);" % twin, text).group(1)
        a = re.sub(r"\s+", " ", a).replace("const uint8_t *pat, size_t plen", "const bzh_patset *set").replace("bzh_hit *", "bzh_set_hit *")
        assert a == re.sub(r"\s+", " ", b), twin


def test_library_exports_and_bindings_mirror_the_header(native):
    assert native.MISSING == []
    L = native.lib()
    for name in FUNCS:
        assert name in native.SIGNATURES and hasattr(L, name), name
    assert native.SET_HIT_DTYPE.itemsize == 24
    assert [(n, native.SET_HIT_DTYPE.fields[n][1]) for n in native.SET_HIT_DTYPE.names] == [("off", 0), ("record", 8), ("pattern", 16), ("len", 20)]
    assert ctypes.sizeof(native.PatsetInfo) == 40
    assert [f for f, _ in native.PatsetInfo._fields_] == ["patterns", "distinct", "min_len", "max_len", "states", "classes", "table_bytes"]
    assert native.PATSET_FOLD_ASCII == 1 and native.PATSET_MAX_PATTERNS == 65536
    for twin in FUNCS[3:]:  # (pat, plen) -> set: one argument fewer
        assert len(native.SIGNATURES[twin][1]) == len(native.SIGNATURES[twin.replace("_patset", "")][1]) - 1, twin
    import banzai_amd
    assert "PatternSet" in banzai_amd.__all__ and issubclass(banzai_amd.PatternSet, native.PatternSet)
    # the calls that need no device
    L.bzh_patset_destroy(None)
    assert L.bzh_patset_get_info(None, ctypes.byref(native.PatsetInfo())) == -1
    assert L.bzh_patset_create(None, None, None, 1, 0, ctypes.byref(ctypes.c_void_p())) == -1


def test_python_surface_refuses_before_the_device(native):
    import banzai_amd
    with pytest.raises(TypeError):
        banzai_amd.PatternSet(["text"])
    with pytest.raises(ValueError):
        banzai_amd.PatternSet([])
    with pytest.raises(ValueError):
        banzai_amd.PatternSet([b"a", b""])
    with pytest.raises(ValueError):
        banzai_amd.PatternSet([b"a", b"x" * 257])
