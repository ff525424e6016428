"""CPU: the surface of the assertions without a device -- what the header declares, that the library exports it and the bindings
mirror it, what bzh_regex_check_ex (the compile alone, pure host) answers with and without the syntax bits, that the calls without
a syntax word refuse what they refused, and what the Python layer refuses before it touches a device."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("bzh_regex_create_ex", "bzh_regex_check_ex", "bzh_regex_get_look")


def test_header_declares_the_assertions():
    text = open(os.path.join(ROOT, "include", "bzhip.h")).read()
    syms = set(re.findall(r"BZH_API[^;(]*?\b(bzh_\w+)\s*\(", text))
    for need in FUNCS:
        assert need in syms, need
    assert re.search(r"enum \{ BZH_REGEX_ASSERT = 1, BZH_REGEX_WORD = 2, BZH_REGEX_LINE = 4 \};", text)
    m = re.search(r"typedef struct \{([^}]*)\}\s*bzh_regex_look;", text)
    assert m, "bzh_regex_look is not declared"
    body = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", m.group(1))).strip()
    assert body == "uint32_t look_behind, look_ahead; uint32_t contexts; uint32_t reserved;"
    sig = lambda name: re.sub(r"/\*.*?\*/", "", re.sub(r"\s+", " ", re.search(r"BZH_API int %s\(([^;]*)\);" % name, text).group(1))).replace("  ", " ")
    assert sig("bzh_regex_create_ex") == ("bzh_ctx *ctx, const uint8_t *const *exprs, const size_t *lens, size_t count, unsigned flags, "
                                          "uint32_t max_span, unsigned syntax, bzh_patset **out")
    assert sig("bzh_regex_check_ex") == ("const uint8_t *const *exprs, const size_t *lens, size_t count, unsigned flags, uint32_t max_span, "
                                         "unsigned syntax, bzh_regex_info *info, bzh_regex_look *look, char *err, size_t errn")
    assert sig("bzh_regex_get_look") == "const bzh_patset *set, bzh_regex_look *out"


def test_library_exports_and_bindings_mirror_the_header(native):
    assert native.MISSING == []
    L = native.lib()
    for name in FUNCS:
        assert name in native.SIGNATURES and hasattr(L, name), name
    assert ctypes.sizeof(native.RegexLook) == 16 and ctypes.sizeof(native.RegexInfo) == 40
    assert (native.REGEX_ASSERT, native.REGEX_WORD, native.REGEX_LINE) == (1, 2, 4)
    assert L.bzh_regex_get_look(None, ctypes.byref(native.RegexLook())) == -1
    assert L.bzh_regex_create_ex(None, None, None, 1, 0, 0, 1, ctypes.byref(ctypes.c_void_p())) == -1


def check(native, exprs, flags=0, span=0, syntax=None):
    arr = (ctypes.c_char_p * max(len(exprs), 1))(*exprs)
    lens = (ctypes.c_size_t * max(len(exprs), 1))(*[len(e) for e in exprs])
    info, look, err = native.RegexInfo(), native.RegexLook(), ctypes.create_string_buffer(b"\xAA" * 200, 200)
    if syntax is None:
        st = native.lib().bzh_regex_check(arr, lens, len(exprs), flags, span, ctypes.byref(info), err, 200)
    else:
        st = native.lib().bzh_regex_check_ex(arr, lens, len(exprs), flags, span, syntax, ctypes.byref(info), ctypes.byref(look), err, 200)
    return st, info.as_dict(), look.as_dict(), err.value.decode("latin-1")


def test_check_ex_is_the_compile_alone(native):
    A, W, X = native.REGEX_ASSERT, native.REGEX_WORD, native.REGEX_LINE
    # a list without assertions: the same figures with and without the bit, and nothing is looked at
    for exprs, flags, span in (([b"abc"], 0, 0), ([b"GET|POST", b"[0-9]{4}", b"err(or)?"], native.REGEX_FOLD_ASCII, 0), ([b"a+"], native.REGEX_NO_LDS, 8)):
        plain, with_bit = check(native, exprs, flags, span), check(native, exprs, flags, span, A)
        assert plain[0] == with_bit[0] == 0 and plain[1] == with_bit[1]
        assert with_bit[2] == {"look_behind": 0, "look_ahead": 0, "contexts": 1}
    # the calls without a syntax word refuse what they refused, with the texts they had
    for exprs, byte, text in (([b"ab", b"^c"], 0, "anchors are not supported"), ([b"ab", b"cd$"], 2, "anchors are not supported"),
                              ([b"a\\b"], 1, "anchors and \\b are not supported"), ([b"\\Aa"], 0, "anchors and \\b are not supported")):
        for syntax in (None, 0):
            st, _, _, err = check(native, exprs, 0, 0, syntax)
            assert st == -1 and err == f"regex: expression {len(exprs) - 1}, byte {byte}: {text}", err
    assert check(native, [b"a"], 8)[0] == -1 and check(native, [b"a"], 8, 0, A)[0] == -1
    # with it
    st, i, look, err = check(native, [b"^ab$"], 0, 0, A)
    assert (st, err) == (0, "") and (i["min_len"], i["max_len"], i["unbounded"]) == (2, 2, 0) and look == {"look_behind": 1, "look_ahead": 1, "contexts": 2}
    st, i, look, _ = check(native, [b"a+$"], 0, 0, A)
    assert st == 0 and (i["min_len"], i["max_len"], i["unbounded"]) == (1, 256, 1) and (look["look_behind"], look["look_ahead"]) == (0, 1)
    st, i, look, _ = check(native, [b"\\bfoo\\b", b"bar"], 0, 0, A)
    assert st == 0 and (i["min_len"], i["max_len"]) == (3, 3) and (look["look_behind"], look["look_ahead"]) == (1, 1)
    st, i, look, _ = check(native, [b"ab"], 0, 0, W)
    assert st == 0 and (look["look_behind"], look["look_ahead"]) == (1, 1) and i["max_len"] == 2
    st, i, look, _ = check(native, [b"ab"], 0, 0, X)
    assert st == 0 and (look["look_behind"], look["look_ahead"]) == (1, 1)
    for exprs, syntax, text in (([b"^"], A, "empty string"), ([b"^$"], A, "empty string"), ([b"\\b"], A, "empty string"), ([b"x", b"a*"], X, "expression 1, byte 0"),
                                ([b"[\\b]"], A, "\\b"), ([b"a^*"], A, "nothing to repeat"), ([b"^a"], W, "anchors"), ([b"a"], W | X, "exclude each other"),
                                ([b"a"], 8, "syntax 0x8"), ([b"a^b"], A, "contradict")):
        st, _, _, err = check(native, exprs, 0, 0, syntax)
        assert st == -1 and text in err, (exprs, err)
    assert native.lib().bzh_regex_check_ex(None, None, 1, 0, 0, 1, None, None, None, 0) == -1


def test_python_surface(native):
    import banzai_amd
    assert banzai_amd.regex_check(b"abc")["look_behind"] == 0 and banzai_amd.regex_check(b"abc")["look_ahead"] == 0
    i = banzai_amd.regex_check([b"^ERROR", b";$"])
    assert (i["look_behind"], i["look_ahead"], i["contexts"], i["min_len"]) == (1, 1, 2, 1)
    assert banzai_amd.regex_check(b"error", word=True)["look_ahead"] == 1 and banzai_amd.regex_check(b"error", line=True)["max_len"] == 5
    with pytest.raises(ValueError) as err:
        banzai_amd.regex_check(b"^")
    assert "empty string" in str(err.value)
    with pytest.raises(ValueError):
        banzai_amd.regex_check(b"a", word=True, line=True)
    with pytest.raises(ValueError):
        banzai_amd.Regex(b"a", word=True, line=True)
