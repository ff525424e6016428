"""CPU: the grep without a device -- what the header declares and the bindings mirror, the room Context._grep gives its calls (a
first try with a guess, a second with the exact rooms), and banzai_amd.grep / grep_count over a fake context.  (The kernel's
layout and the windows run against a naive split-and-find in tests/test_grep_host.py.)"""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = {"bzh_grep_raw_device": 13, "bzh_grep_device": 15, "bzh_grep": 15, "bzh_grep_index_device": 17, "bzh_grep_index": 17,
         "bzh_get_grep_stats": 2}


def test_header_declares_grep():
    text = open(os.path.join(ROOT, "include", "bzhip.h")).read()
    decl = {m.group(1): m.group(2) for m in re.finditer(r"BZH_API[^;(]*?\b(bzh_\w+)\s*\(([^;]*)\);", text)}
    for need, nargs in FUNCS.items():
        assert need in decl and decl[need].count(",") + 1 == nargs, need
    flat = " ".join(re.sub(r"\n \* ", " ", text).split())
    for phrase in ("} bzh_grep_entry; /* 32 bytes */", "enum { BZH_GREP_INVERT = 1 };", "uint64_t record;", "uint64_t out_off;",
                   "A record is HIT when a match of pat starts inside it", "belongs to the record of its first byte",
                   "a pattern may contain the delimiter", "in ascending record order", "a selected tail comes as it is",
                   "*nrecs (selected records) and *out_total (their bytes) are always exact", "never causes BZH_E_CAP",
                   "is a counting call and returns BZH_OK", "repeating the call with the exact room succeeds",
                   "a d_out that is not 4-byte aligned", "d_raw must be 16-byte aligned", "The call is all or nothing",
                   "every error text are bzh_decode's", "block and stream CRCs are verified", "stream CRCs are not checked, as there",
                   "npts == 0: one wavefront a block", "It needs no record table", "record numbers count from 0",
                   "an input without any delimiter holds all of its output in the carry",
                   "No read goes past the aligned 4-byte word that holds byte n - 1",
                   "no store goes outside out[0, *out_total), ent[0, *nrecs) and the kernel's own tables",
                   "Every workgroup copies only bytes of its own tile", "honour bzh_set_profiling",
                   "leave the context usable after any outcome"):
        assert phrase in flat, phrase
    # the section stands behind the search section and in front of the encoder's index
    assert text.index("bzh_get_search_stats(") < text.index("bzh_grep_raw_device(") < text.index("bzh_get_grep_stats(") < \
        text.index("bzh_encode_index_device(")
    for field in ("records", "selected", "out_bytes", "windows", "tiles", "carry_peak", "staging_peak"):
        assert re.search(r"uint64_t %s;[^}]*} bzh_grep_stats;" % field, text), field


def test_bindings_mirror_the_header(native):
    L = native.lib()
    assert native.MISSING == []
    for name, nargs in FUNCS.items():
        assert name in native.SIGNATURES and hasattr(L, name), name
        assert len(native.SIGNATURES[name][1]) == nargs, name
    assert native.GREP_ENTRY_DTYPE.itemsize == 32 and native.GREP_ENTRY_DTYPE.names == ("record", "off", "len", "out_off")
    assert native.ctypes.sizeof(native.GrepEntry) == 32 and native.GREP_INVERT == 1
    assert [k for k, _ in native.GrepStats._fields_] == ["records", "selected", "out_bytes", "windows", "tiles", "carry_peak", "staging_peak"]
    for attr in ("grep", "grep_device", "grep_raw_device", "grep_index", "grep_stats"):
        assert hasattr(native.Context, attr)
    import banzai_amd
    for name in ("grep", "grep_count"):
        assert name in banzai_amd.__all__ and hasattr(banzai_amd, name)
    # the sources: the kernels' file is built, the shared texts are headers of their own, nothing is counted with atomics
    mk = open(os.path.join(ROOT, "banzai_amd", "csrc", "Makefile")).read()
    assert "grep.hip" in mk
    kern = open(os.path.join(ROOT, "banzai_amd", "csrc", "grep.hip")).read()
    assert '#include "grep_core.h"' in kern and "grep_tiles<false>" in kern and "grep_tiles<true>" in kern and "grep_scan<<<" in kern
    assert "atomicAdd" not in kern and "atomic" not in open(os.path.join(ROOT, "banzai_amd", "csrc", "grep_core.h")).read()
    assert '#include "search_core.h"' in open(os.path.join(ROOT, "banzai_amd", "csrc", "grep_core.h")).read()
    host = open(os.path.join(ROOT, "tests", "decode_host", "grep_host.cpp")).read()
    assert "grep_core.h" in host and "grep_plan.h" in host


# ---- the room of a call -----------------------------------------------------------------------------------------------------------
def fake_call(records, log):
    """a C call that knows the selected records: fills what fits, says BZH_E_CAP when a room that is asked for is too small"""
    data = b"".join(records)

    def call(out, cap, ent, room, got, total):
        log.append((cap, room))
        got._obj.value, total._obj.value = len(records), len(data)
        over = (out is not None and cap < len(data)) or (ent is not None and room < len(records))
        if not over:
            at = 0
            for k, r in enumerate(records):
                if ent is not None:
                    ent[k].record, ent[k].off, ent[k].len, ent[k].out_off = 3 * k, 100 + at, len(r), at
                at += len(r)
            if out is not None:
                for k, b in enumerate(data):
                    out[k] = b
        return -4 if over else 0
    return call


def test_grep_room(native):
    ctx = native.Context.__new__(native.Context)  # (no device: _grep talks to the call it is given)
    ctx._h = None
    ctx.GREP_GUESS = (16, 3)
    for records in ([], [b"a\n"], [b"abc\n"] * 3, [b"abcd\n"] * 3 + [b"x"], [b"a\n"] * 4, [b"0123456789abcde\n", b"tail"]):
        log = []
        data, ent = ctx._grep(fake_call(records, log))
        want = b"".join(records)
        assert data == want and len(ent) == len(records) and ent.dtype == native.GREP_ENTRY_DTYPE
        assert ent["record"].tolist() == [3 * k for k in range(len(records))] and ent["len"].tolist() == [len(r) for r in records]
        assert [data[int(e["out_off"]):int(e["out_off"]) + int(e["len"])] for e in ent] == records
        fits = len(want) <= 16 and len(records) <= 3
        assert log == ([(16, 3)] if fits else [(16, 3), (len(want), len(records))])
        log = []
        assert ctx._grep(fake_call(records, log), count_only=True) == (len(records), len(want)) and log == [(0, 0)]
    grow = iter([[b"a\n"] * 5, [b"a\n"] * 6])  # the second call selects more than the first said
    with pytest.raises(native.BzhError):
        ctx._grep(lambda *a: fake_call(next(grow), [])(*a))


# ---- banzai_amd.grep / grep_count over a fake context ------------------------------------------------------------------------------
class FakeContext:
    def __init__(self, native, truth):
        self.native, self.truth, self.calls = native, truth, []

    def _answer(self, pattern, delim, invert, count_only):
        d = bytes([delim])
        cut = self.truth.split(d)
        recs = [p + d for p in cut[:-1]] + ([cut[-1]] if cut[-1] else [])
        out, ent, off = bytearray(), [], 0
        for k, r in enumerate(recs):
            # a match belongs to the record of its first byte: it starts inside the record, and may end behind it
            hit = any(self.truth.startswith(pattern, s) for s in range(off, off + len(r)))
            if hit != invert:
                ent.append((k, off, len(r), len(out)))
                out += r
            off += len(r)
        if count_only:
            return len(ent), len(out)
        return bytes(out), np.array(ent, dtype=self.native.GREP_ENTRY_DTYPE)

    def grep(self, data, pattern, delim=b"\n", invert=False, count_only=False):
        self.calls.append(("grep", bytes(data), None))
        return self._answer(pattern, delim, invert, count_only)

    def grep_index(self, comp, entries, pattern, points=None, delim=b"\n", invert=False, count_only=False):
        self.calls.append(("grep_index", bytes(comp), points is not None))
        return self._answer(pattern, delim, invert, count_only)


def test_grep_over_a_fake_context(native, monkeypatch):
    import banzai_amd
    truth = b"alpha beta\ngamma\n\nbeta beta alpha\nbetabeta\nno newline at the end: beta"
    source = bytes(range(256)) * 2
    fake = FakeContext(native, truth)
    monkeypatch.setattr(banzai_amd, "_ctx", lambda level, device=0: fake)
    data, ent = banzai_amd.grep(source, b"beta")
    lines = truth.split(b"\n")
    want = [k for k, line in enumerate(lines) if b"beta" in line]
    assert ent["record"].tolist() == want and data == b"".join(lines[k] + (b"\n" if k < len(lines) - 1 else b"") for k in want)
    assert ent.dtype.names == ("record", "off", "len", "out_off") and fake.calls[-1] == ("grep", source, None)
    assert banzai_amd.grep_count(source, b"beta") == len(want)
    inv, ient = banzai_amd.grep(source, b"beta", invert=True)
    assert sorted(ent["record"].tolist() + ient["record"].tolist()) == list(range(len(lines))) and len(data) + len(inv) == len(truth)
    assert banzai_amd.grep(source, b"a\ngam")[1]["record"].tolist() == [0]  # the record of the match's first byte
    assert banzai_amd.grep(source, b" ", delim=b"a")[1]["record"].tolist() == banzai_amd.grep(source, b" ", delim=ord("a"))[1]["record"].tolist()
    e = np.zeros(2, dtype=native.INDEX_DTYPE)
    e[0] = (32, 832, 0, 40, 0x1000, 0, 9)
    e[1] = (832, 1640, 40, len(truth) - 40, 0x1001, 0, 9)
    blocks = banzai_amd.BlockIndex(e, len(source))
    assert banzai_amd.grep(source, b"beta", index=blocks)[0] == data and fake.calls[-1] == ("grep_index", source, False)
    assert banzai_amd.grep_count(source, b"beta", invert=True, index=blocks) == len(ient)
    for bad in (b"", b"x" * 257):
        with pytest.raises(ValueError):
            banzai_amd.grep(source, bad)
    with pytest.raises(TypeError):
        banzai_amd.grep(source, "beta")
    with pytest.raises(TypeError):
        banzai_amd.grep(source, b"beta", index=e)
    for bad in (b"ab", 256, None, "x"):
        with pytest.raises(ValueError):
            banzai_amd.grep(source, b"beta", delim=bad)
    with pytest.raises(ValueError):
        native.Context._grep_args(b"a", None, False)
    assert hasattr(banzai_amd.IndexedReader, "grep")
