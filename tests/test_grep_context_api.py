"""CPU: context records for the grep without a device -- what the header declares and the bindings mirror
(bzh_grep_set_context, bzh_get_grep_context_stats, BZH_GREP_LEN_CONTEXT), the argument errors of banzai_amd.grep and
IndexedReader.grep, and those of bnzhip's -A / -B / -C.  (The phases and the windows run against a naive split-find-dilate in
tests/test_grep_context_host.py.)"""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = {"bzh_grep_set_context": 3, "bzh_get_grep_context_stats": 2}


def test_header_declares_the_context():
    text = open(os.path.join(ROOT, "include", "bzhip.h")).read()
    decl = {m.group(1): m.group(2) for m in re.finditer(r"BZH_API[^;(]*?\b(bzh_\w+)\s*\(([^;]*)\);", text)}
    for need, nargs in FUNCS.items():
        assert need in decl and decl[need].count(",") + 1 == nargs, need
    assert "uint32_t before, uint32_t after" in decl["bzh_grep_set_context"]
    assert re.search(r"#define BZH_GREP_LEN_CONTEXT \(1ull << 63\)", text)
    for field in ("matched", "context", "groups", "pending_peak"):
        assert re.search(r"uint64_t %s;[^}]*} bzh_grep_context_stats;" % field, text), field
    # the entry and the flags stay as they are: no new flag bit
    assert "} bzh_grep_entry;     /* 32 bytes */" in text and "enum { BZH_GREP_INVERT = 1 };" in text
    assert text.index("bzh_get_grep_stats(") < text.index("bzh_grep_set_context(") < text.index("bzh_get_grep_context_stats(")


def test_bindings_mirror_the_header(native):
    L, c = native.lib(), native.ctypes
    assert native.MISSING == []
    for name, nargs in FUNCS.items():
        assert name in native.SIGNATURES and hasattr(L, name) and len(native.SIGNATURES[name][1]) == nargs, name
    assert native.SIGNATURES["bzh_grep_set_context"][1][1:] == [c.c_uint32, c.c_uint32]
    assert native.GREP_LEN_CONTEXT == 1 << 63
    assert [k for k, _ in native.GrepContextStats._fields_] == ["matched", "context", "groups", "pending_peak"]
    assert c.sizeof(native.GrepContextStats) == 32
    assert native.GREP_CONTEXT_ENTRY_DTYPE.names == ("record", "off", "len", "out_off", "context")
    ent = np.zeros(3, dtype=native.GREP_ENTRY_DTYPE)
    ent["record"], ent["len"], ent["out_off"] = [4, 5, 9], [7, 3 | 1 << 63, 1 << 63], [0, 7, 10]
    got = native.grep_context_rows(ent)
    assert got["len"].tolist() == [7, 3, 0] and got["context"].tolist() == [False, True, True] and got["record"].tolist() == [4, 5, 9]
    for attr in ("grep_set_context", "grep_context_stats"):
        assert hasattr(native.Context, attr)
    # a null context is an argument error, not a crash
    assert L.bzh_grep_set_context(None, 1, 1) == -1
    assert L.bzh_get_grep_context_stats(None, c.byref(native.GrepContextStats())) == -1
    # the sources: the context phases are a header of their own beside grep_core.h, and nothing is counted with atomics
    kern = open(os.path.join(ROOT, "banzai_amd", "csrc", "grep.hip")).read()
    core = open(os.path.join(ROOT, "banzai_amd", "csrc", "grep_ctx_core.h")).read()
    assert '#include "grep_ctx_core.h"' in kern and "grep_ctx_tiles<<<" in kern and "grep_ctx_scan<<<" in kern
    assert "atomicAdd" not in kern and "atomicAdd" not in core and '#include "grep_core.h"' in core
    host = open(os.path.join(ROOT, "tests", "decode_host", "grep_ctx_host.cpp")).read()
    assert "grep_ctx_plan.h" in host and "scan_host.h" in host


class Recorder:
    """a context that records what banzai_amd.grep hands it"""

    def __init__(self, native):
        self.native, self.calls = native, []

    def grep(self, data, pattern, delim=b"\n", invert=False, count_only=False, **kw):
        self.calls.append(("grep", kw))
        return (0, 0) if count_only else (b"", np.zeros(0, dtype=self.native.GREP_CONTEXT_ENTRY_DTYPE if kw else self.native.GREP_ENTRY_DTYPE))

    def grep_index(self, comp, entries, pattern, points=None, delim=b"\n", invert=False, count_only=False, **kw):
        self.calls.append(("grep_index", kw))
        return self.grep(comp, pattern, delim, invert, count_only, **kw)


def test_python_arguments(native, monkeypatch):
    import banzai_amd
    fake = Recorder(native)
    monkeypatch.setattr(banzai_amd, "_ctx", lambda level, device=0: fake)
    src = b"BZh9" + bytes(40)
    assert banzai_amd.grep(src, b"a")[1].dtype == native.GREP_ENTRY_DTYPE and fake.calls[-1] == ("grep", {})  # today's call, today's dtype
    assert banzai_amd.grep(src, b"a", before=0, after=0, context=0)[1].dtype == native.GREP_ENTRY_DTYPE and fake.calls[-1] == ("grep", {})
    assert banzai_amd.grep(src, b"a", before=2)[1].dtype == native.GREP_CONTEXT_ENTRY_DTYPE and fake.calls[-1] == ("grep", {"before": 2, "after": 0})
    banzai_amd.grep(src, b"a", after=3)
    assert fake.calls[-1] == ("grep", {"before": 0, "after": 3})
    banzai_amd.grep(src, b"a", context=5)
    assert fake.calls[-1] == ("grep", {"before": 5, "after": 5})
    banzai_amd.grep(src, b"a", context=np.int64(4), invert=True)
    assert fake.calls[-1] == ("grep", {"before": 4, "after": 4})
    for kw in ({"before": 1, "context": 1}, {"after": 1, "context": 1}, {"before": -1}, {"after": -1}, {"context": -1}, {"before": 1.0},
               {"after": "1"}, {"context": 2.5}, {"before": True}, {"after": 1 << 32}, {"before": None}):
        with pytest.raises(ValueError):
            banzai_amd.grep(src, b"a", **kw)
    import inspect
    sig = inspect.signature(banzai_amd.grep)
    assert list(sig.parameters) == ["data", "pattern", "delim", "invert", "index", "device", "before", "after", "context"]
    assert [sig.parameters[k].default for k in ("before", "after", "context")] == [0, 0, None]
    assert list(inspect.signature(banzai_amd.grep_count).parameters) == ["data", "pattern", "delim", "invert", "index", "device"]
    assert list(inspect.signature(banzai_amd.IndexedReader.grep).parameters) == ["self", "pattern", "limit", "before", "after"]


def test_wrappers_reset_the_setting(native):
    """Context.grep sets the context for its call and resets it, whatever the call does"""
    ctx = native.Context.__new__(native.Context)
    log = []
    ctx.grep_set_context = lambda b, a: log.append((b, a))
    ent = np.zeros(1, dtype=native.GREP_ENTRY_DTYPE)
    ent["len"] = 5 | 1 << 63
    data, got = ctx._grep_with_context(2, 0, lambda: (b"abcd\n", ent))
    assert log == [(2, 0), (0, 0)] and got.dtype == native.GREP_CONTEXT_ENTRY_DTYPE and got["len"].tolist() == [5] and got["context"].tolist() == [True]
    assert ctx._grep_with_context(0, 1, lambda: (3, 17)) == (3, 17) and log[2:] == [(0, 1), (0, 0)]  # a counting call
    with pytest.raises(RuntimeError):
        ctx._grep_with_context(1, 1, lambda: (_ for _ in ()).throw(RuntimeError("the call failed")))
    assert log[4:] == [(1, 1), (0, 0)]
    assert ctx._grep_with_context(0, 0, lambda: (b"", ent))[1].dtype == native.GREP_ENTRY_DTYPE and len(log) == 6


def test_cli_arguments(tmp_path):
    exe = os.path.join(ROOT, "banzai_amd", "bnzhip")
    f = tmp_path / "t.bz2"
    f.write_bytes(b"")
    run = lambda *args: subprocess.run([exe, *args], capture_output=True, text=True, timeout=60)
    for args, text in ((("-A", "2", str(f)), "'-A', '-B' and '-C' go with '--grep'"),
                       (("--search", "x", "-C", "1", str(f)), "'-A', '-B' and '-C' go with '--grep'"),
                       (("--context", "1", "-d", str(f)), "'-A', '-B' and '-C' go with '--grep'"),
                       (("--grep", "x", str(f), "-A"), "require a number of lines"),
                       (("--grep", "x", "-B", "-1", str(f)), "require a number of lines"),
                       (("--grep", "x", "-C", "two", str(f)), "require a number of lines"),
                       (("--grep", "x", "--after-context", "4294967296", str(f)), "require a number of lines"),
                       (("--grep", "x", "-A", "1", "-d", str(f)), "'-A', '-B', '-C' and '--index', nothing else")):
        p = run(*args)
        assert p.returncode != 0 and text in p.stderr, (args, p.stderr)
    p = run("--help")
    usage = p.stdout + p.stderr
    for opt in ("-A --after-context <n>", "-B --before-context <n>", "-C --context <n>", "'-' on a context line"):
        assert opt in usage, opt
