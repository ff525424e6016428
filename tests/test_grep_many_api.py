"""CPU: the grep over many inputs without a device -- what the header declares and the bindings mirror, what the C calls refuse
before a device is touched, the rooms Context.grep_many gives its calls, and banzai_amd.grep_many / grep_many_count over a fake
context.  (The virtual-tile plan and the kernels' phases run against a naive split-and-find in tests/test_grep_many_host.py.)"""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = {"bzh_grep_many_raw_device": 17, "bzh_grep_many_device": 17, "bzh_grep_many": 15, "bzh_grep_many_patset_raw_device": 16,
         "bzh_grep_many_patset_device": 16, "bzh_grep_many_patset": 14, "bzh_get_grep_many_stats": 2}
STATS = ["inputs", "inputs_failed", "segments", "virtual_tiles", "shared_tiles", "staging_retries"]


def test_header_declares_grep_many():
    text = open(os.path.join(ROOT, "include", "bzhip.h")).read()
    decl = {m.group(1): m.group(2) for m in re.finditer(r"BZH_API[^;(]*?\b(bzh_\w+)\s*\(([^;]*)\);", text)}
    for need, nargs in FUNCS.items():
        assert need in decl and decl[need].count(",") + 1 == nargs, need
    flat = " ".join(re.sub(r"\n \* ", " ", text).split())
    for phrase in ("} bzh_grep_many_item; /* 40 bytes */", "uint64_t decoded;", "int32_t status;", "uint32_t reserved;",
                   "exactly what bzh_grep returns for input k alone", "a match starts and ends inside one input",
                   "record numbers and `off` restart at 0 with every input", "as the text's edges", "a damaged input fails alone",
                   "nothing is gathered, BZH_E_CAP", "The segments ascend and do not overlap; gaps are allowed and never scanned",
                   "BZH_E_ARG naming the segment", "never returns BZH_E_CAP for its own staging", "count == 0 succeeds",
                   "an input shorter than a tile still costs a tile's work", "No atomics; one host wait before the gather"):
        assert phrase in flat, phrase
    for field in STATS:
        assert re.search(r"uint64_t [^;]*\b%s\b[^}]*} bzh_grep_many_stats;" % field, text), field
    assert text.index("bzh_get_match_stats(") < text.index("bzh_grep_many_raw_device(") < text.index("bzh_encode_index_device(")


def test_bindings_mirror_the_header(native):
    L = native.lib()
    assert native.MISSING == []
    for name, nargs in FUNCS.items():
        assert name in native.SIGNATURES and hasattr(L, name), name
        assert len(native.SIGNATURES[name][1]) == nargs, name
    assert native.GREP_MANY_ITEM_DTYPE.itemsize == ctypes.sizeof(native.GrepManyItem) == 40
    assert native.GREP_MANY_ITEM_DTYPE.names == ("decoded", "records", "selected", "out_bytes", "status", "reserved")
    assert [k for k, _ in native.GrepManyStats._fields_] == STATS
    for attr in ("grep_many", "grep_many_device", "grep_many_raw_device", "grep_many_stats"):
        assert hasattr(native.Context, attr)
    import banzai_amd
    for name in ("grep_many", "grep_many_count"):
        assert name in banzai_amd.__all__ and hasattr(banzai_amd, name)
    # the older twins still get their names
    assert native._patset_twin("bzh_grep_raw_device") == "bzh_grep_patset_raw_device" and native._patset_twin("bzh_match") == "bzh_match_patset"
    assert native._patset_twin("bzh_search_range") == "bzh_search_patset_range"
    assert native._patset_twin("bzh_grep_many") == "bzh_grep_many_patset"
    # the sources: the kernels' file is built, it runs the shared phases, nothing is counted with atomics
    csrc = os.path.join(ROOT, "banzai_amd", "csrc")
    assert "grep_many.hip" in open(os.path.join(csrc, "Makefile")).read()
    kern = open(os.path.join(csrc, "grep_many.hip")).read()
    assert "grep_many_tiles<false>" in kern and "grep_many_tiles<true>" in kern and "grep_many_scan<<<" in kern
    for phase in ("bzg_masks(", "bzg_count_p1(", "bzg_gather_p3(", "bzg_scan_a(", "bzg_scan_e(", "bzgm_close(", "bzgm_rebind("):
        assert phase in kern, phase
    core = open(os.path.join(csrc, "grep_many_core.h")).read()
    assert '#include "grep_core.h"' in core and "atomic" not in kern.replace("No atomics", "") and "atomic" not in core
    plan = open(os.path.join(csrc, "grep_many_plan.h")).read()
    assert "hip" not in plan.replace("bzhip", "").replace("grep_many.hip", "").lower(), "the plan is pure host text"
    host = open(os.path.join(ROOT, "tests", "decode_host", "grep_many_host.cpp")).read()
    assert "grep_many_plan.h" in host and "int main(" in host


def test_refused_before_a_device_is_touched(native):
    L = native.lib()
    n1 = ctypes.c_size_t(7)
    tot = ctypes.c_uint64(7)
    pat = (ctypes.c_uint8 * 2)(97, 98)
    items = (native.GrepManyItem * 1)()
    one = (ctypes.c_size_t * 1)(0)
    # no context: BZH_E_ARG from every entry point, and nothing is written
    assert L.bzh_grep_many_raw_device(None, None, 0, one, one, 1, pat, 2, 0, 10, None, 0, None, 0, items, ctypes.byref(n1), ctypes.byref(tot)) == -1
    assert L.bzh_grep_many_device(None, None, 0, one, one, 1, pat, 2, 0, 10, None, 0, None, 0, items, ctypes.byref(n1), ctypes.byref(tot)) == -1
    assert L.bzh_grep_many(None, None, one, 0, pat, 2, 0, 10, None, 0, None, 0, items, ctypes.byref(n1), ctypes.byref(tot)) == -1
    assert L.bzh_grep_many_patset_raw_device(None, None, 0, one, one, 1, None, 0, 10, None, 0, None, 0, items, ctypes.byref(n1), ctypes.byref(tot)) == -1
    assert L.bzh_grep_many_patset_device(None, None, 0, one, one, 1, None, 0, 10, None, 0, None, 0, items, ctypes.byref(n1), ctypes.byref(tot)) == -1
    assert L.bzh_grep_many_patset(None, None, one, 0, None, 0, 10, None, 0, None, 0, items, ctypes.byref(n1), ctypes.byref(tot)) == -1
    assert L.bzh_get_grep_many_stats(None, None) == -1
    assert n1.value == 7 and tot.value == 7
    # the wrappers look at their arguments before any C call
    ctx = native.Context.__new__(native.Context)
    ctx._h = None
    with pytest.raises(ValueError):
        ctx.grep_many_raw_device(0, 0, [0, 1], [1], b"a", 0, 0, 0)
    with pytest.raises(ValueError):
        ctx.grep_many_raw_device(0, 0, [0], [1], b"a", 0, 0, 0, delim=None)


# ---- the rooms of Context.grep_many, over a fake C call ---------------------------------------------------------------------------
def test_grep_many_rooms_and_items(native, monkeypatch):
    per_input = [[b"ab\n", b"cab"], None, [], [b"xab\n"] * 3]  # the selected records of every input; None: a damaged one
    log = []

    def fake_raw(self, inputs, pattern, cap, room, delim=b"\n", invert=False):
        log.append((cap, room))
        recs = [r for p in per_input if p for r in p]
        data = b"".join(recs)
        items = np.zeros(len(per_input), dtype=native.GREP_MANY_ITEM_DTYPE)
        for k, p in enumerate(per_input):
            items[k] = (0, 0, 0, 0, -6, 0) if p is None else (100, 9, len(p), sum(map(len, p)), 0, 0)
        over = (cap and cap < len(data)) or (room and room < len(recs))
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        ent = np.zeros(0 if over else min(room, len(recs)), dtype=native.GREP_ENTRY_DTYPE)
        if not over and cap:
            out[:len(data)] = np.frombuffer(data, dtype=np.uint8)
            at = 0
            for k, r in enumerate(recs):
                ent[k] = (k % 3, 10 * k, len(r), at)
                at += len(r)
        return (-4 if over else 0), len(recs), len(data), out, ent, items

    monkeypatch.setattr(native.Context, "grep_many_host_raw", fake_raw)
    ctx = native.Context.__new__(native.Context)
    ctx._h = None
    for guess, calls in (((64, 8), [(64, 8)]), ((4, 8), [(4, 8), (18, 5)]), ((64, 2), [(64, 2), (18, 5)])):
        ctx.GREP_GUESS = guess
        del log[:]
        items, res = ctx.grep_many([b"."] * 4, b"ab")
        assert log == calls
        assert items["status"].tolist() == [0, -6, 0, 0] and res[1] is None
        assert res[0][0] == b"ab\ncab" and res[2][0] == b"" and res[3][0] == b"xab\n" * 3
        assert [len(r[1]) for r in res if r] == [2, 0, 3]
        # every input's out_off counts from its own first byte, as bzh_grep of it alone numbers them
        assert res[0][1]["out_off"].tolist() == [0, 3] and res[3][1]["out_off"].tolist() == [0, 4, 8]
    del log[:]
    items, res = ctx.grep_many([b"."] * 4, b"ab", count_only=True)
    assert res is None and log == [(0, 0)] and items["selected"].tolist() == [2, 0, 0, 3]


# ---- banzai_amd.grep_many / grep_many_count over a fake context ---------------------------------------------------------------------
class FakeMany:
    def __init__(self, native, texts):
        self.native, self.texts, self.calls = native, texts, []

    def last_error(self):
        return "decode: input 1: a damaged block"

    def grep_many(self, inputs, pattern, delim=10, invert=False, count_only=False):
        self.calls.append(len(inputs))
        items = np.zeros(len(inputs), dtype=self.native.GREP_MANY_ITEM_DTYPE)
        res = []
        for k, x in enumerate(inputs):
            t = self.texts[bytes(x)]
            if t is None:
                items[k]["status"] = -6
                res.append(None)
                continue
            lines = [ln for ln in t.splitlines(True) if (pattern in ln) != invert]
            items[k]["selected"] = len(lines)
            res.append((b"".join(lines), np.zeros(len(lines), dtype=self.native.GREP_ENTRY_DTYPE)))
        return items, (None if count_only else res)


def test_grep_many_over_a_fake_context(native, monkeypatch):
    import banzai_amd
    texts = {b"A": b"error one\nfine\nerror two", b"B": None, b"C": b"", b"D": b"nothing\n"}
    fake = FakeMany(native, texts)
    monkeypatch.setattr(banzai_amd, "_ctx", lambda level, device=0: fake)
    assert banzai_amd.grep_many([], b"error") == [] and fake.calls == []
    got = banzai_amd.grep_many([b"A", b"C", b"D"], b"error")
    assert [g[0] for g in got] == [b"error one\nerror two", b"", b""] and fake.calls == [3]
    assert banzai_amd.grep_many_count([b"A", b"C", b"D"], b"error") == [2, 0, 0]
    assert banzai_amd.grep_many_count([b"A", b"D"], b"error", invert=True) == [1, 1]
    with pytest.raises(native.BzhError) as e:
        banzai_amd.grep_many([b"A", b"B", b"D"], b"error")
    assert e.value.status == -6 and "item 1 of grep_many" in str(e.value)
    got = banzai_amd.grep_many([b"A", b"B", b"D"], b"error", errors="return")
    assert isinstance(got[1], native.BzhError) and got[1].status == -6 and got[0][0] == b"error one\nerror two" and got[2][0] == b""
    assert isinstance(banzai_amd.grep_many_count([b"B", b"A"], b"error", errors="return")[0], native.BzhError)
    # groups below MANY_GROUP_LIMIT bytes, as decompress_many's
    monkeypatch.setattr(banzai_amd, "MANY_GROUP_LIMIT", 4)
    del fake.calls[:]
    assert banzai_amd.grep_many_count([b"A", b"C", b"D", b"A"], b"error") == [2, 0, 0, 2] and fake.calls == [2, 2]
    with pytest.raises(ValueError):
        banzai_amd.grep_many([b"A"], b"error", errors="ignore")
    with pytest.raises(ValueError):
        banzai_amd.grep_many([b"A"], b"")
    with pytest.raises(TypeError):
        banzai_amd.grep_many([b"A"], "error")
    with pytest.raises(TypeError):
        banzai_amd.grep_many(["A"], b"error")
