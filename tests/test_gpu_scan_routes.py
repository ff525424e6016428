"""GPU: the thirty entry points of the scan family -- bzh_search*, bzh_grep*, bzh_match*, each for a byte string and for a
PatternSet, each through its five routes (decoded bytes in HBM, compressed on the device, compressed on the host, indexed on the
device, indexed on the host) -- held to ONE behaviour where they are meant to have one.  The refusal matrix drives the C calls
themselves (native.lib()): which status, which message, whether the caller's count words were zeroed before the refusal or keep
their poison, and whether the family's statistics were cleared or left alone.  The agreement check runs every route over one
input with a match across every seam and asks for byte-identical answers, equal to a plain Python model."""
import bisect
import bz2
import ctypes
import re

import numpy as np
import pytest

from tests.test_gpu_grep import find_all, on_device, room_on_device
from tests.test_gpu_match import prose

pytestmark = pytest.mark.gpu

POISON = 0x5A5A5A5A
ROUTES = ("raw_device", "device", "host", "index_device", "index_host")
NAMES = {
    "search": ("bzh_search_raw_device", "bzh_search_device", "bzh_search", "bzh_search_range_device", "bzh_search_range"),
    "grep": ("bzh_grep_raw_device", "bzh_grep_device", "bzh_grep", "bzh_grep_index_device", "bzh_grep_index"),
    "match": ("bzh_match_raw_device", "bzh_match_device", "bzh_match", "bzh_match_index_device", "bzh_match_index"),
}
FLAG_NAME = {"search": "BZH_SEARCH_RECORDS", "grep": "BZH_GREP_INVERT", "match": "BZH_MATCH_RECORDS"}
E_ARG, E_CAP = -1, -4
INTS = (ctypes.c_size_t, ctypes.c_uint64, ctypes.c_uint, ctypes.c_uint8, ctypes.c_uint32)


def small_text(first):
    """newline-terminated rows, a needle in every seventh, two in every twenty-first"""
    rows = []
    for k in range(first, first + 60):
        rows.append(b"row %d holds a needle and a needle\n" % k if k % 21 == 3 else b"row %d holds a needle here\n" % k if k % 7 == 3
                    else b"row %d is filler xyz\n" % k)
    return b"".join(rows)


class World:
    """what the matrix calls with: a context, a small input of two streams in every form the routes take, rooms, and the truth"""

    def __init__(self, native):
        self.nv = native
        self.dec = native.Context(0, 9, 2)
        self.text = small_text(0) + small_text(60)
        self.s = bz2.compress(small_text(0), 9) + bz2.compress(small_text(60), 9)
        assert bz2.decompress(self.s) == self.text
        self.ent, self.pts, total, _ = self.dec.decode_index_sync(self.s, 4)
        assert len(self.ent) == 2 and total == len(self.text)
        self.bad_ent = self.ent.copy()
        self.bad_ent[1]["bit_pos"] = self.ent[0]["bit_pos"]  # "bit_pos does not ascend"
        self.pset = native.PatternSet(self.dec, [b"needle"])
        self.pat = np.frombuffer(b"needle" + bytes(506), dtype=np.uint8).copy()
        self.d_raw, self.d_comp = on_device(self.text), on_device(self.s)
        assert self.d_raw.data_ptr() % 16 == 0 and self.d_comp.data_ptr() % 16 == 0
        self.h_comp = np.frombuffer(self.s, dtype=np.uint8).copy()
        self.d_out = room_on_device(len(self.text))
        self.h_out = np.zeros(len(self.text) + 16, dtype=np.uint8)
        self.h_ent = np.zeros(32 * 256, dtype=np.uint8)  # room for 256 entries or hits of any kind
        hits = find_all(self.text, b"needle")
        recs = [r + b"\n" for r in self.text.split(b"\n")[:-1] if b"needle" in r]
        self.truth = {"search": (len(hits), None), "grep": (len(recs), sum(map(len, recs))), "match": (len(hits), 6 * len(hits))}
        assert len(hits) > len(recs) > 4

    def close(self):
        self.pset.close()
        self.dec.close()

    def stats(self, fam):
        if fam == "search":
            return self.dec.search_stats()
        if fam == "grep":
            return {**self.dec.grep_stats(), **{"context " + k: v for k, v in self.dec.grep_context_stats().items()}}
        return self.dec.match_stats()

    def call(self, fam, what, route, ctx=True, count=True, total=True, skew=0, idx="good", nidx=None, pat=True, plen=6, pset=True,
             flags=0, rec_cum=None, out=None, cap=0, ent=False, room=0):
        """one C call -> (status, the count word, the out_total word (None: a search has none), last_error()).  Pointers travel as
        integer addresses and become what the call's argtypes say; out: None, "room" (the route's own kind of buffer) or an address"""
        name = NAMES[fam][ROUTES.index(route)]
        fn = getattr(self.nv.lib(), name if what == "bytes" else self.nv._patset_twin(name))
        host, indexed = route in ("host", "index_host"), route.startswith("index")
        if host:
            src, n = self.h_comp.ctypes.data, self.h_comp.size
        else:
            t = self.d_raw if route == "raw_device" else self.d_comp
            src, n = t.data_ptr() + skew, (len(self.text) if route == "raw_device" else len(self.s)) - skew
        got, tot = ctypes.c_size_t(POISON), ctypes.c_uint64(POISON)
        e = {"good": self.ent, "bad": self.bad_ent, None: None}[idx]
        args = [self.dec.handle.value if ctx else None, src, n]
        if indexed:
            args += ([0] if fam == "search" else []) + [e.ctypes.data if e is not None else None, len(self.ent) if nidx is None else nidx,
                                                          self.pts.ctypes.data, len(self.pts)]
            args += [rec_cum, 0, 2**64 - 1] if fam == "search" else []
        args += [self.pat.ctypes.data if pat else None, plen] if what == "bytes" else [self.pset.handle.value if pset else None]
        args += [flags, 10]
        if fam != "search":
            if out == "room":
                out = self.h_out.ctypes.data if host else self.d_out.data_ptr()
            args += [out, cap]
        args += [self.h_ent.ctypes.data if ent else None, room, ctypes.addressof(got) if count else None]
        if fam != "search":
            args += [ctypes.addressof(tot) if total else None]
        if route in ("device", "host"):
            args += [None, None]
        assert len(args) == len(fn.argtypes), name
        conv = [v if t in INTS else None if v is None else ctypes.cast(ctypes.c_void_p(v), t) for v, t in zip(args, fn.argtypes)]
        st = fn(*conv)
        return st, int(got.value), (int(tot.value) if fam != "search" else None), self.dec.last_error()


@pytest.fixture(scope="module")
def world(native):
    w = World(native)
    yield w
    w.close()


def refusals(fam, what, route):
    """-> [(case, arguments of World.call, status, are the count words zeroed, are the stats cleared, what the message holds)];
    a message is asked for only where the call sets one"""
    word = fam + ":"
    out = [
        ("null context", dict(ctx=False), E_ARG, False, False, ()),
        ("null count pointer", dict(count=False), E_ARG, False, False, ()),
        ("null array, room for 1", dict(ent=False, room=1), E_ARG, False, False, ()),
        ("nothing to look for", dict(pat=False, pset=False), E_ARG, False, False, ()),
        ("an undefined flag bit", dict(flags=2), E_ARG, True, False, (word, FLAG_NAME[fam])),
        ("the family's flag and an undefined bit", dict(flags=3), E_ARG, True, False, (word, FLAG_NAME[fam])),
    ]
    if what == "bytes":
        out += [("pattern length 0", dict(plen=0), E_ARG, True, False, (word, "outside 1..256")),
                ("pattern length 257", dict(plen=257), E_ARG, True, False, (word, "outside 1..256"))]
    if fam != "search":
        out += [("null out_total pointer", dict(total=False), E_ARG, False, False, ()),
                ("null output, room for 1 byte", dict(out=None, cap=1), E_ARG, False, False, ())]
        if route in ("raw_device", "device", "index_device"):
            out.append(("output misaligned by 2", dict(out="skew", cap=64), E_ARG, True, False, (word, "4-byte aligned")))
    if route == "raw_device":
        out.append(("input misaligned by 1", dict(skew=1), E_ARG, True, True, (word, "16-byte aligned")))
    if route.startswith("index"):
        out += [("entries counted, null index", dict(idx=None, nidx=1), E_ARG, False, False, ()),
                ("second entry ill formed", dict(idx="bad"), E_ARG, True, True, ("index entry 1", "bit_pos does not ascend"))]
        if fam == "search":
            out.append(("record numbers without a table", dict(flags=1, rec_cum=None), E_ARG, True, True, ("search range:", "no record table")))
    return out


@pytest.mark.parametrize("fam", list(NAMES))
def test_refusals_and_rooms_of_every_entry_point(world, fam):
    w, bad = world, []
    nwant, twant = w.truth[fam]
    for what in ("bytes", "set"):
        for route in ROUTES:
            who = (fam, what, route)
            # the counting call: every room 0
            st, got, tot, _ = w.call(fam, what, route)
            if (st, got, tot) != (0, nwant, twant):
                bad.append((who, "counting call", st, got, tot))
            primed = w.stats(fam)
            assert any(primed.values()), who
            for case, kw, status, zeroed, cleared, phrases in refusals(fam, what, route):
                if kw.get("out") == "skew":
                    kw = dict(kw, out=w.d_out.data_ptr() + 2)
                if not any(w.stats(fam).values()):  # (the last refusal cleared them)
                    assert w.call(fam, what, route)[0] == 0
                before = w.stats(fam)
                st, got, tot, msg = w.call(fam, what, route, **kw)
                after = w.stats(fam)
                words = [v for v, there in ((got, kw.get("count", True)), (tot, fam != "search" and kw.get("total", True))) if there]
                if st != status:
                    bad.append((who, case, "status", st))
                if any(v != (0 if zeroed else POISON) for v in words):
                    bad.append((who, case, "count words", got, tot, "zeroed" if zeroed else "poison"))
                if (not any(after.values())) != cleared or (not cleared and after != before):
                    bad.append((who, case, "stats", before, after))
                if any(p not in msg for p in phrases):
                    bad.append((who, case, "message", msg))
            # an array with no room: a search counts, a grep and a match were asked for entries and have room for none
            st, got, tot, msg = w.call(fam, what, route, ent=True, room=0)
            if (st, got, tot) != (0 if fam == "search" else E_CAP, nwant, twant) or (st and "room for" not in msg):
                bad.append((who, "array with room 0", st, got, tot, msg))
            # one slot too few
            st, got, tot, msg = w.call(fam, what, route, ent=True, room=nwant - 1, out="room" if fam != "search" else None, cap=twant or 0)
            if (st, got, tot) != (E_CAP, nwant, twant) or fam + ":" not in msg or "room for" not in msg:
                bad.append((who, "one slot too few", st, got, tot, msg))
            # the exact rooms
            st, got, tot, msg = w.call(fam, what, route, ent=True, room=nwant, out="room" if fam != "search" else None, cap=twant or 0)
            if (st, got, tot) != (0, nwant, twant):
                bad.append((who, "the exact rooms", st, got, tot, msg))
    assert not bad, "\n".join(map(repr, bad))


# ---- every route over one input ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dec1(native):
    """batches of one candidate and a room of 1024 bytes: the chain route and the indexed routes hand every block over as a window
    of its own"""
    c = native.Context(0, 9, 1)
    c.search_set_room(1024)
    yield c
    c.close()


class Words:
    """tests/test_gpu_match.py's input -- two streams, a level-1 one of two blocks and one of one block -- with a stretch of
    "ab ab ab ..." across the block edge and across the stream edge: a match of either thing looked for at every third byte, no
    delimiter, so the record, the matches and what an assertion looks at all cross both edges; computed once, never changed"""

    def __init__(self, dec):
        parts = [bytearray(prose(150_000, 31)), bytearray(prose(12_000, 32))]
        pack = lambda: b"".join(bz2.compress(bytes(p), 1 if k == 0 else 9) for k, p in enumerate(parts))
        ent = dec.decode_index(pack())[0]
        assert len(ent) == 3
        bounds = [int(e["out_off"]) for e in ent[1:]]
        assert bounds[1] == len(parts[0])
        whole = bytearray(b"".join(parts))
        for b in bounds:
            whole[b - 8301:b + 8300] = (b"ab " * 5534)[:16601]
        parts = [whole[:bounds[1]], whole[bounds[1]:]]
        self.s = pack()
        self.truth = bz2.decompress(self.s)
        assert self.truth == bytes(whole)
        self.ent, self.pts, total, _ = dec.decode_index_sync(self.s, 4)
        self.bounds = [int(e["out_off"]) for e in self.ent[1:]]  # (a block is cut where a run ends: a bound may move by a byte or two)
        assert len(self.ent) == 3 and all(abs(a - b) < 100 for a, b in zip(self.bounds, bounds)) and total == len(whole) and len(self.pts) > 4
        for a in (self.ent, self.pts):
            a.setflags(write=False)


@pytest.fixture(scope="module")
def inp(dec1):
    """with the input its record table, the decoded bytes and the compressed bytes on the device"""
    i = Words(dec1)
    i.d_raw, i.d_comp = on_device(i.truth), on_device(i.s)
    i.cum = dec1.count_records_device(i.d_raw.data_ptr(), len(i.truth), i.ent, 10)[0]
    i.newlines = [k for k, b in enumerate(i.truth) if b == 10]
    return i


WHATS = {"ab": (lambda nv, d: b"ab", lambda t: find_all(t, b"ab")),
         r"\bab\b": (lambda nv, d: nv.PatternSet(d, [rb"\bab\b"], regex=True, syntax=nv.REGEX_ASSERT),
                     lambda t: [m.start() for m in re.finditer(rb"\bab\b", t)])}


@pytest.mark.parametrize("name", list(WHATS))
@pytest.mark.parametrize("fam", list(NAMES))
def test_the_five_routes_agree(dec1, inp, native, fam, name):
    what, starts = WHATS[name][0](native, dec1), WHATS[name][1](inp.truth)
    assert len(starts) > 5000 and all(any(abs(s - b) < 3 for s in starts) for b in inp.bounds)  # (a match on every edge)
    d_raw, d_comp, n, nc = inp.d_raw.data_ptr(), inp.d_comp.data_ptr(), len(inp.truth), len(inp.s)
    windows = []
    if fam == "search":
        stats = dec1.search_stats
        runs = [lambda: dec1.search_raw_device(d_raw, n, what, b"\n"), lambda: dec1.search_device(d_comp, nc, what, b"\n"),
                lambda: dec1.search(inp.s, what, b"\n"),
                lambda: dec1.search_range(nc, inp.ent, what, points=inp.pts, rec_cum=inp.cum, delim=b"\n", d_in=d_comp),
                lambda: dec1.search_range(inp.s, inp.ent, what, points=inp.pts, rec_cum=inp.cum, delim=b"\n")]
        got = []
        for run in runs:
            hits, nhits = run()
            assert nhits == len(hits)
            got.append(hits.tobytes())
            windows.append(stats()["windows"])
        assert [int(v) for v in hits["off"]] == starts and [int(v) for v in hits["record"]] == [bisect.bisect_left(inp.newlines, s) for s in starts]
        if name != "ab":
            assert set(hits["len"].tolist()) == {2} and set(hits["pattern"].tolist()) == {0}
    else:
        if fam == "grep":
            stats = dec1.grep_stats
            host, idx_host = lambda: dec1.grep(inp.s, what), lambda: dec1.grep_index(inp.s, inp.ent, what, inp.pts)
            raw, dev, idx_dev = dec1.grep_raw_device, dec1.grep_device, dec1.grep_index_device
            offs, want, rows = [0] + [k + 1 for k in inp.newlines], bytearray(), []
            assert offs[-1] == n  # (the text ends with a newline: no open tail in the model)
            for k in sorted({bisect.bisect_right(offs, s) - 1 for s in starts}):
                rows.append((k, offs[k], offs[k + 1] - offs[k], len(want)))
                want += inp.truth[offs[k]:offs[k + 1]]
            fields = ("record", "off", "len", "out_off")
        else:
            stats = dec1.match_stats
            host, idx_host = lambda: dec1.matches(inp.s, what, b"\n"), lambda: dec1.matches_index(inp.s, inp.ent, what, inp.pts, b"\n")
            raw, dev, idx_dev = dec1.match_raw_device, dec1.match_device, dec1.match_index_device
            want = b"ab" * len(starts)
            rows = [(s, bisect.bisect_left(inp.newlines, s), 0, 2, 2 * k) for k, s in enumerate(starts)]
            fields = ("off", "record", "pattern", "len", "out_off")
        data, ent = host()
        windows.append(stats()["windows"])
        assert data == bytes(want) and [tuple(int(e[f]) for f in fields) for e in ent] == rows
        got = [(data, ent.tobytes())]
        data, ent = idx_host()
        windows.append(stats()["windows"])
        got.append((data, ent.tobytes()))
        for k, run in enumerate((lambda o: raw(d_raw, n, what, o.data_ptr(), len(want), len(rows), b"\n"),
                                 lambda o: dev(d_comp, nc, what, o.data_ptr(), len(want), len(rows), b"\n"),
                                 lambda o: idx_dev(d_comp, nc, inp.ent, what, o.data_ptr(), len(want), len(rows), inp.pts, b"\n"))):
            out = room_on_device(len(want))
            st, cnt, total, ent = run(out)
            assert (st, cnt, total) == (0, len(rows), len(want)), (k, dec1.last_error())
            mem = out.cpu().numpy().tobytes()
            assert set(mem[len(want):]) <= {0xA5}
            got.append((mem[:len(want)], ent.tobytes()))
            windows.append(stats()["windows"])
        windows.pop(2)  # (the raw route: one window)
    assert all(g == got[0] for g in got), [k for k, g in enumerate(got) if g != got[0]]
    if fam == "search":
        windows.pop(0)
    assert all(wn >= 3 for wn in windows), windows  # every block a window of its own: block edge and stream edge were window edges
    if hasattr(what, "close"):
        what.close()
