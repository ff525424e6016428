"""CPU: the regular expressions' surface without a device -- what the header declares, that the built library exports it, that
the bindings mirror it, what bzh_regex_check (the compile alone, pure host) answers, and what the Python layer refuses before it
touches a device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("bzh_regex_create", "bzh_regex_get_info", "bzh_regex_check")


def header():
    return open(os.path.join(ROOT, "include", "bzhip.h")).read()


def test_header_declares_the_regex():
    text = header()
    syms = set(re.findall(r"BZH_API[^;(]*?\b(bzh_\w+)\s*\(", text))
    for need in FUNCS:
        assert need in syms, need
    assert re.search(r"enum \{ BZH_REGEX_FOLD_ASCII = 1, BZH_REGEX_DOTALL = 2, BZH_REGEX_NO_LDS = 4 \};", text)
    assert re.search(r"#define BZH_REGEX_MAX_SPAN 256\b", text) and re.search(r"#define BZH_REGEX_MAX_EXPR 4096\b", text)
    m = re.search(r"typedef struct \{([^}]*)\}\s*bzh_regex_info;", text)
    assert m, "bzh_regex_info is not declared"
    body = re.sub(r"/\*.*?\*/", "", m.group(1))
    assert re.sub(r"\s+", " ", body).strip() == ("uint64_t expressions; uint32_t min_len, max_len; uint32_t states, classes; "
                                                 "uint32_t unbounded, in_lds; uint64_t table_bytes;")
    sig = lambda name: re.sub(r"/\*.*?\*/", "", re.sub(r"\s+", " ", re.search(r"BZH_API int %s\(([^;]*)\);" % name, text).group(1))).replace("  ", " ")
    assert sig("bzh_regex_create") == ("bzh_ctx *ctx, const uint8_t *const *exprs, const size_t *lens, size_t count, unsigned flags, "
                                       "uint32_t max_span , bzh_patset **out")
    assert sig("bzh_regex_get_info") == "const bzh_patset *set, bzh_regex_info *out"
    assert sig("bzh_regex_check") == ("const uint8_t *const *exprs, const size_t *lens, size_t count, unsigned flags, uint32_t max_span, "
                                      "bzh_regex_info *info, char *err, size_t errn")
    # additions only: the pattern set's info stays as it was
    m = re.search(r"typedef struct \{([^}]*)\}\s*bzh_patset_info;", text)
    assert re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", m.group(1))).strip() == ("uint64_t patterns, distinct; uint32_t min_len, max_len; "
                                                                                  "uint32_t states, classes; uint64_t table_bytes;")


def test_library_exports_and_bindings_mirror_the_header(native):
    assert native.MISSING == []
    L = native.lib()
    for name in FUNCS:
        assert name in native.SIGNATURES and hasattr(L, name), name
    assert ctypes.sizeof(native.RegexInfo) == 40
    assert [f for f, _ in native.RegexInfo._fields_] == ["expressions", "min_len", "max_len", "states", "classes", "unbounded", "in_lds", "table_bytes"]
    assert (native.REGEX_FOLD_ASCII, native.REGEX_DOTALL, native.REGEX_NO_LDS, native.REGEX_MAX_SPAN, native.REGEX_MAX_EXPR) == (1, 2, 4, 256, 4096)
    import banzai_amd
    assert "Regex" in banzai_amd.__all__ and issubclass(banzai_amd.Regex, native.PatternSet)
    # the calls that need no device
    assert L.bzh_regex_get_info(None, ctypes.byref(native.RegexInfo())) == -1
    assert L.bzh_regex_create(None, None, None, 1, 0, 0, ctypes.byref(ctypes.c_void_p())) == -1


def check(native, exprs, flags=0, span=0):
    arr = (ctypes.c_char_p * max(len(exprs), 1))(*exprs)
    lens = (ctypes.c_size_t * max(len(exprs), 1))(*[len(e) for e in exprs])
    info, err = native.RegexInfo(), ctypes.create_string_buffer(b"\xAA" * 200, 200)
    st = native.lib().bzh_regex_check(arr, lens, len(exprs), flags, span, ctypes.byref(info), err, 200)
    return st, info.as_dict(), err.value.decode("latin-1")


def test_regex_check_is_the_compile_alone(native):
    st, i, err = check(native, [b"abc"])
    assert (st, err) == (0, "") and (i["expressions"], i["min_len"], i["max_len"], i["unbounded"]) == (1, 3, 3, 0)
    assert i["table_bytes"] == 2 * i["states"] * i["classes"] and i["in_lds"] == 1
    st, i, err = check(native, [b"a+"])
    assert st == 0 and (i["min_len"], i["max_len"], i["unbounded"]) == (1, 256, 1)
    st, i, err = check(native, [b"a+"], native.REGEX_NO_LDS, 8)
    assert st == 0 and (i["min_len"], i["max_len"], i["unbounded"], i["in_lds"]) == (1, 8, 1, 0)
    st, i, err = check(native, [b"GET|POST", b"[0-9]{4}", b"err(or)?"], native.REGEX_FOLD_ASCII)
    assert st == 0 and (i["expressions"], i["min_len"], i["max_len"], i["unbounded"]) == (3, 3, 5, 0)
    for exprs, span, byte, text in (([b"a{3}"], 2, 0, "max_span 2"), ([b"a*"], 0, 0, "empty string"), ([b"ab", b"^c"], 0, 0, "anchors"),
                                    ([b"ab", b"cd$"], 0, 2, "anchors"), ([b"a\\b"], 0, 1, "\\b"), ([b"(a)\\1"], 0, 3, "backreferences"),
                                    ([b"a(?=b)"], 0, 1, "lookaround"), ([b"a+?"], 0, 2, "lazy"), ([b"a*+"], 0, 2, "possessive"),
                                    ([b"(?P<n>a)"], 0, 0, "named groups"), ([b"(?i)a"], 0, 0, "inline flags"), ([b"ab{"], 0, 2, "well-formed bound"),
                                    ([b"a{,2}"], 0, 1, "well-formed bound"), ([b"a{257}"], 0, 1, "bound above 256"), ([b"x[abc"], 0, 1, "unbalanced bracket"),
                                    ([b"x(ab"], 0, 1, "unbalanced bracket"), ([b"xab)"], 0, 3, "unbalanced bracket"),
                                    ([b"(a|b)*a(a|b){16}"], 0, None, "states")):
        st, _, err = check(native, exprs, 0, span)
        assert st == -1 and text in err, (exprs, err)
        if byte is not None:
            assert f"expression {len(exprs) - 1}, byte {byte}:" in err, (exprs, err)
    assert check(native, [])[0] == -1 and check(native, [b"a"], 8)[0] == -1 and check(native, [b"a"], 0, 257)[0] == -1
    assert native.lib().bzh_regex_check(None, None, 1, 0, 0, None, None, 0) == -1  # no room for the reason is allowed


def test_python_surface_refuses_before_the_device(native):
    import banzai_amd
    with pytest.raises(TypeError):
        banzai_amd.Regex("text")
    with pytest.raises(TypeError):
        banzai_amd.Regex(["text"])
    with pytest.raises(ValueError):
        banzai_amd.Regex([])
    with pytest.raises(ValueError):
        banzai_amd.Regex([b"a", b""])
    with pytest.raises(ValueError):
        banzai_amd.Regex(b"")
    with pytest.raises(ValueError):
        banzai_amd.Regex([b"a", b"x" * 4097])
    with pytest.raises(ValueError):
        banzai_amd.Regex(b"a", max_span=0)
    with pytest.raises(ValueError):
        banzai_amd.Regex(b"a", max_span=257)
    with pytest.raises(ValueError) as err:
        banzai_amd.regex_check([b"ok", b"a**"])
    assert "expression 1, byte 2" in str(err.value)
    assert banzai_amd.regex_check(b"x" * 256)["max_len"] == 256 and banzai_amd.regex_check([b"a.c"], dotall=True)["classes"] == 3
