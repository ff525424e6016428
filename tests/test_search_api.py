"""CPU: the search without a device -- what the header declares and the bindings mirror, the room Context._search gives its calls
(a first try, a second with the exact room, a limit that makes BZH_E_CAP the answer), and banzai_amd.search_range /
IndexedReader.search / grep over a fake back end that searches the truth with plain Python: the span that is fetched, the
arguments that reach the call, the records grep asks for.  (The windows and the carry of search_plan.h run against brute force in
tests/test_search_host.py.)"""
import io
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = {"bzh_search_raw_device": 10, "bzh_search_device": 12, "bzh_search": 12, "bzh_search_range_device": 18, "bzh_search_range": 18,
         "bzh_search_set_room": 2, "bzh_get_search_stats": 2}


def test_header_declares_search():
    text = open(os.path.join(ROOT, "include", "bzhip.h")).read()
    syms = set(re.findall(r"BZH_API[^;(]*?\b(bzh_\w+)\s*\(", text))
    for need in FUNCS:
        assert need in syms
    flat = " ".join(re.sub(r"\n \* ", " ", text).split())
    for phrase in ("typedef struct { uint64_t off;", "enum { BZH_SEARCH_RECORDS = 1 };", "#define BZH_SEARCH_MAX_PATTERN 256",
                   "overlapping ones included", "Hits are reported in ascending off", "*nhits is always the exact number of hits",
                   "hits[0 .. max) hold the first max hits", "is a counting call and returns BZH_OK", "d_raw must be 16-byte aligned",
                   "A pattern longer than the output has no hits", "no hit is trusted until the call returns BZH_OK or BZH_E_CAP",
                   "record table does not match entry e", "as WHOLE blocks into staging", "A window always holds whole blocks and at least one block",
                   "belongs to the record of its first byte"):
        assert phrase in flat, phrase
    # the section stands behind the records section
    assert text.index("bzh_decode_records(") < text.index("bzh_search_raw_device(") < text.index("bzh_encode_index_device(")


def test_bindings_mirror_the_header(native):
    L = native.lib()
    assert native.MISSING == []
    for name, nargs in FUNCS.items():
        assert name in native.SIGNATURES and hasattr(L, name), name
        assert len(native.SIGNATURES[name][1]) == nargs, name
    assert native.HIT_DTYPE.itemsize == 16 and native.HIT_DTYPE.names == ("off", "record")
    assert native.SEARCH_RECORDS == 1 and native.SEARCH_MAX_PATTERN == 256
    for attr in ("search", "search_device", "search_raw_device", "search_range", "search_set_room", "search_stats"):
        assert hasattr(native.Context, attr)
    import banzai_amd
    for name in ("search", "search_range"):
        assert name in banzai_amd.__all__ and hasattr(banzai_amd, name)
    assert hasattr(banzai_amd.IndexedReader, "search") and hasattr(banzai_amd.IndexedReader, "grep")
    # the sources: the kernel's file is built, the shared texts are headers of their own
    mk = open(os.path.join(ROOT, "banzai_amd", "csrc", "Makefile")).read()
    assert "search.hip" in mk
    kern = open(os.path.join(ROOT, "banzai_amd", "csrc", "search.hip")).read()
    assert '#include "search_core.h"' in kern and "search_tiles<false>" in kern and "search_tiles<true>" in kern and "atomicAdd" not in kern
    host = open(os.path.join(ROOT, "tests", "decode_host", "search_host.cpp")).read()
    assert "search_core.h" in host and "search_plan.h" in host


# ---- the room of a call -----------------------------------------------------------------------------------------------------------
def fake_call(total, log):
    """a C call that knows `total` hits (i, 2 i): fills what fits, says BZH_E_CAP when max is not 0 and too small"""
    def call(hits, room, got):
        log.append(room)
        got._obj.value = total
        for i in range(min(room, total)):
            hits[i].off, hits[i].record = i, 2 * i
        return -4 if 0 < room < total else 0
    return call


def test_search_room(native):
    ctx = native.Context.__new__(native.Context)  # (no device: _search talks to the call it is given)
    ctx._h = None
    ctx.SEARCH_GUESS = 8
    for total in (0, 3, 8, 9, 40):
        log = []
        hits, n = ctx._search(fake_call(total, log), None)
        assert n == total and hits["off"].tolist() == list(range(total)) and hits["record"].tolist() == [2 * i for i in range(total)]
        assert log == ([8] if total <= 8 else [8, total])
        for limit in (0, 1, total, total + 3):
            log = []
            hits, n = ctx._search(fake_call(total, log), limit)
            assert n == total and hits["off"].tolist() == list(range(min(limit, total))) and log == [limit]
            assert ctx.search_status == (-4 if 0 < limit < total else 0)
    with pytest.raises(ValueError):
        ctx._search(fake_call(1, []), -1)
    assert native.Context._delim(None) == (0, 0) and native.Context._delim(b"\n") == (1, 10) and native.Context._delim(0) == (1, 0)
    for bad in (b"ab", 256, -1, "x"):
        with pytest.raises(ValueError):
            native.Context._delim(bad)


# ---- search_range, IndexedReader.search and grep over a fake back end --------------------------------------------------------------
def make_index(native, truth, sizes, delim=10):
    e = np.zeros(len(sizes), dtype=native.INDEX_DTYPE)
    cum = np.zeros(len(sizes) + 1, dtype=np.uint64)
    bit, off = 32, 0
    for k, size in enumerate(sizes):
        e[k] = (bit, bit + 800 + 8 * k, off, size, 0x1000 + k, 0, 1)
        bit += 800 + 8 * k
        cum[k + 1] = cum[k] + truth[off:off + size].count(bytes([delim]))
        off += size
    assert off == len(truth)
    return e, cum


def find_all(truth, pat, lo, hi):
    out, at = [], truth.find(pat, lo, hi)
    while at >= 0:
        out.append(at)
        at = truth.find(pat, at + 1, hi)
    return out


class FakeContext:
    """bzh_search_range by plain Python over the truth; checks that the bytes it is handed are the span of the range"""

    def __init__(self, native, truth, source):
        self.native, self.truth, self.source, self.calls = native, truth, source, []

    def search_range(self, comp, entries, pattern, off=0, length=None, points=None, rec_cum=None, delim=None, limit=None, in_byte_base=0):
        first, last, lo, hi = self.native.index_span(entries, off, length)
        assert in_byte_base == lo and bytes(comp) == self.source[lo:hi], "exactly the span's bytes are handed over"
        assert (rec_cum is None) == (delim is None)
        self.calls.append((off, length, limit))
        end = min(off + length, len(self.truth))
        found = find_all(self.truth, pattern, off, end)
        hits = np.zeros(len(found) if limit is None else min(limit, len(found)), dtype=self.native.HIT_DTYPE)
        hits["off"] = found[:len(hits)]
        if delim is not None:
            hits["record"] = [self.truth.count(bytes([delim]), 0, o) for o in found[:len(hits)]]
        return hits, len(found)

    def decode_records(self, comp, entries, rec_cum, ranges, points=None, in_byte_base=0, delim=10):
        cut = self.truth.split(bytes([delim]))
        recs = [p + bytes([delim]) for p in cut[:-1]] + [cut[-1]]
        parts = [b"".join(recs[a:a + c]) for a, c in ranges]
        offs = [sum(len(p) for p in parts[:i]) for i in range(len(parts))]
        return b"".join(parts), offs, [len(p) for p in parts]


class CountingFile(io.BytesIO):
    def __init__(self, data):
        super().__init__(data)
        self.reads = []

    def read(self, n=-1):
        self.reads.append((self.tell(), n))
        return super().read(n)


def test_reader_search_and_grep_over_a_fake_back_end(native, monkeypatch):
    import banzai_amd
    truth = b"alpha beta\ngamma\n\nbeta beta alpha\nbetabeta\nno newline at the end: beta"
    sizes = [7, 9, 1, 20, len(truth) - 37]
    e, cum = make_index(native, truth, sizes)
    source = bytes(range(256)) * 3  # (the compressed bytes are only fetched and handed over here)
    nrec = truth.count(b"\n") + 1
    rindex = banzai_amd.RecordIndex(banzai_amd.BlockIndex(e, len(source)), b"\n", cum, nrec)
    fake = FakeContext(native, truth, source)
    monkeypatch.setattr(banzai_amd, "_ctx", lambda level, device=0: fake)
    for index in (rindex, rindex.index):
        delim = 10 if index is rindex else None
        for off, length in ((0, None), (0, len(truth)), (3, 30), (16, 1), (len(truth), 5), (len(truth) + 9, None), (11, 2**64 - 1)):
            hits, n = banzai_amd.search_range(source, index, b"beta", off, length)
            end = len(truth) if length is None else min(off + length, len(truth))
            want = find_all(truth, b"beta", off, end)
            assert n == len(want) and hits["off"].tolist() == want
            assert hits["record"].tolist() == [truth.count(b"\n", 0, o) if delim else 0 for o in want]
    f = CountingFile(source)
    rd = banzai_amd.IndexedReader(f, rindex)
    hits, n = rd.search(b"beta", 8, 30, limit=1)
    assert n == 2 and hits["off"].tolist() == [18] and fake.calls[-1] == (8, 22, 1)
    _, _, lo, hi = native.index_span(e, 8, 22)
    assert f.reads == [(lo, hi - lo)] and rd.tell() == 0
    got = rd.grep(b"beta")
    lines = truth.split(b"\n")
    want = [k for k, line in enumerate(lines) if b"beta" in line]
    assert [r for r, _ in got] == want and [b for _, b in got] == [lines[k] + (b"\n" if k < len(lines) - 1 else b"") for k in want]
    assert rd.grep(b"delta") == []
    # a match that spans a delimiter belongs to the record of its first byte
    assert [r for r, _ in rd.grep(b"a\ngam")] == [0]
    with pytest.raises(ValueError):
        banzai_amd.IndexedReader(source, rindex.index).grep(b"beta")
    for bad in (b"", b"x" * 257):
        with pytest.raises(ValueError):
            banzai_amd.search_range(source, rindex, bad)
    with pytest.raises(TypeError):
        banzai_amd.search_range(source, rindex, "beta")
    with pytest.raises(TypeError):
        banzai_amd.search_range(source, e, b"beta")
    with pytest.raises(ValueError):
        banzai_amd.search_range(source, rindex, b"beta", -1)
