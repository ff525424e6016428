"""GPU: regular expressions for search and grep, a DFA walked on the device (bzh_regex_*, banzai_amd.Regex, bnzhip -E), through
every bzh_search_patset* and bzh_grep_patset* route.  Every comparison is against Python's `re` under the rule of
tests/regex_truth.py: one hit a start, the longest match of at most max_span bytes, the lowest-numbered expression of that length.
The context takes batches of 2 candidates, so the blocks of the full input are several batches."""
import bz2
import functools
import os
import random
import re
import subprocess

import numpy as np
import pytest

from tests import regex_truth as truth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = (0, 1, 15, 16, 17, 4095, 4096, 4097, 8192, 12289)
GRID = [(b"[0-9]+", 256), (b"err(or)?.*time", 256), (b"(abc)+|a{2,3}", 256), (b"\\s+", 256), (b"[^a]+", 256), (b".+", 16), (b"a+", 256)]
WORDS = [b"abc", b"aa", b"a", b"err", b"ERROR", b"error", b"time", b"Time", b" ", b"\n", b"\t ", b"12", b"7", b"x", b"cd", b"ab", b"ABC", b"A"]


def text_of(n, seed):
    r, out = random.Random(seed), bytearray()
    while len(out) < n:
        out += r.choice(WORDS)
    return bytes(out[:n])


def rows(found, text, delim=10):
    """truth.hits -> [(off, record, pattern, len)]"""
    cuts = np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == delim) if delim is not None else None
    return [(o, int(np.searchsorted(cuts, o)) if delim is not None else 0, p, n) for o, p, n in found]


def hit_rows(hits):
    return [tuple(int(h[f]) for f in ("off", "record", "pattern", "len")) for h in hits]


def ent_rows(entries):
    return [tuple(int(e[f]) for f in ("record", "off", "len", "out_off")) for e in entries]


def grep_rows(found, text, invert=False, delim=b"\n"):
    """-> (bytes, [(record, off, len, out_off)]) of the records in which a hit starts"""
    live, out, ent, start, k = {h[0] for h in found}, bytearray(), [], 0, 0
    while start < len(text):
        end = text.find(delim, start)
        end = len(text) if end < 0 else end + 1
        if any(s in live for s in range(start, end)) != invert:
            ent.append((k, start, end - start, len(out)))
            out += text[start:end]
        start, k = end, k + 1
    return bytes(out), ent


@pytest.fixture(scope="module")
def dec(native):
    c = native.Context(0, 9, 2)
    yield c
    c.close()


def rx(native, dec, exprs, flags=0, span=0):
    return native.PatternSet(dec, exprs, flags=flags, regex=True, max_span=span)


def on_device(data):
    import torch
    t = torch.frombuffer(bytearray(data) or bytearray(1), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return t


def room_on_device(cap):
    import torch
    t = torch.full((max(cap, 1) + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


def search_raw_call(native, dec, t, n, pset, flags, delim, room):
    """bzh_search_patset_raw_device with exactly `room` hit slots in front of two that nobody may touch -> (status, nhits, hits)"""
    c = native.ctypes
    hits = np.full(room + 2, 0xA5, dtype=np.uint8).repeat(24).view(native.SET_HIT_DTYPE)
    got = c.c_size_t(0)
    st = native.lib().bzh_search_patset_raw_device(dec.handle, t.data_ptr(), n, pset.handle, flags, delim, hits.ctypes.data_as(c.c_void_p) if room else None,
                                                   room, c.byref(got))
    assert hits[room:].tobytes() == b"\xA5" * 48, "a hit slot behind the room was written"
    return st, int(got.value), hits[:room]


def raw_search(native, dec, src, pset, want):
    t = on_device(src)
    st, n0, _ = search_raw_call(native, dec, t, len(src), pset, 1, 10, 0)  # the counting call
    assert (st, n0) == (0, len(want)), len(src)
    st, n1, hits = search_raw_call(native, dec, t, len(src), pset, 1, 10, len(want))
    assert (st, n1) == (0, len(want)) and hit_rows(hits) == want, len(src)
    ss = dec.search_stats()
    assert ss["windows"] == 1 and ss["tiles"] == (len(src) + 4095) // 4096 and ss["hits"] == len(want)


def raw_grep(dec, src, pset, found, invert):
    want, ent = grep_rows(found, src, invert)
    t = on_device(src)
    st, nrecs, total, _ = dec.grep_raw_device(t.data_ptr(), len(src), pset, 0, 0, 0, b"\n", invert)  # the counting call
    assert (st, nrecs, total) == (0, len(ent), len(want)), (len(src), invert)
    out = room_on_device(len(want))
    st, nrecs, total, got = dec.grep_raw_device(t.data_ptr(), len(src), pset, out.data_ptr(), len(want), len(ent), b"\n", invert)
    host = out.cpu().numpy().tobytes()
    assert (st, nrecs, total) == (0, len(ent), len(want)) and host[:len(want)] == want and set(host[len(want):]) <= {0xA5}, (len(src), invert)
    assert ent_rows(got) == ent


def raw_all(native, dec, src, exprs, flags=0, span=256):
    found = truth.hits(exprs, src, flags, span)
    with rx(native, dec, exprs, flags, span) as pset:
        raw_search(native, dec, src, pset, rows(found, src))
        raw_grep(dec, src, pset, found, False)
        raw_grep(dec, src, pset, found, True)
    return found


# ---- the raw seam ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("case", range(len(GRID)))
def test_raw_grid(dec, native, case, fold):
    expr, span = GRID[case]
    found = 0
    for n in NS:
        found += len(raw_all(native, dec, text_of(n, n + case), [expr], truth.FOLD if fold else 0, span))
    assert found > 200


def test_raw_planted_places(dec, native):
    """a match of exactly max_span bytes that ends at byte n - 1; one that starts at 15, at 1023 and at 4095; one of 256 bytes from
    4095 to the halo's last byte; the delimiter inside a match"""
    for n in (4500, 12289):
        src = bytearray(b"." * n)
        src[n - 256:] = b"x" * 256
        for at in (15, 1023, 4095):
            src[at:at + 6] = b"Q0451Z"
        src = bytes(src)
        found = raw_all(native, dec, src, [b"x+", b"Q[0-9]+Z"])
        assert (n - 256, 0, 256) in found and (n - 257, 0, 256) not in found and {(15, 1, 6), (1023, 1, 6), (4095, 1, 6)} <= set(found)
    src = bytearray(b"." * 8192)
    src[4095:4095 + 256] = b"x" * 256
    src[100:103], src[5000:5004] = b" \n\t", b"\n\n \n"
    found = raw_all(native, dec, bytes(src), [b"x+", b"\\s+"])
    assert (4095, 0, 256) in found and (4096, 0, 255) in found and (100, 1, 3) in found and (5000, 1, 4) in found and (5002, 1, 2) in found


@pytest.mark.parametrize("span", [256, 8])
def test_raw_equal_bytes(dec, native, span):
    """300 equal bytes under x+: every start reports min(max_span, what is left); every slot, three and none"""
    src = b"x" * 300
    found = raw_all(native, dec, src, [b"x+"], 0, span)
    assert found == [(s, 0, min(span, 300 - s)) for s in range(300)]
    with rx(native, dec, [b"X+"], truth.FOLD, span) as pset:
        assert pset.info["max_len"] == span and pset.info["unbounded"] == 1
        t = on_device(src)
        st, nh, hits = search_raw_call(native, dec, t, 300, pset, 1, ord("x"), 3)
        assert (st, nh) == (-4, 300) and hit_rows(hits) == [(s, s, 0, span) for s in range(3)]
        st, nh, _ = search_raw_call(native, dec, t, 300, pset, 0, 0, 0)
        assert (st, nh) == (0, 300)


def test_the_lower_number_wins_the_longest_length(dec, native):
    src = b"..abc..abd..ab.." * 40
    for exprs in ([b"ab|abc", b"abc", b"a[a-c]c", b"abd?"], [b"abd?", b"a[a-c]c", b"abc", b"ab|abc"]):
        found = raw_all(native, dec, src, exprs)
        assert found[:3] == [(2, 0 if exprs[0] == b"ab|abc" else 1, 3), (7, exprs.index(b"abd?"), 3), (12, 0, 2)]


@functools.lru_cache(maxsize=None)
def many_words():
    rng = random.Random(5)
    return [bytes(rng.choice(b"abcdefgh") for _ in range(rng.randrange(3, 9))) for _ in range(300)]


def test_rows_in_lds_and_in_hbm(dec, native):
    """one automaton that every workgroup stages into LDS, one above the bound (an alternation of 300 words), and the first
    again with BZH_REGEX_NO_LDS: the same hits"""
    rng = random.Random(6)
    src = bytes(rng.choice(b"abcdefgh \n") for _ in range(12289))
    big = [b"|".join(many_words()[:150]), b"|".join(many_words()[150:])]
    with rx(native, dec, big) as pset:
        assert pset.info["in_lds"] == 0 and pset.info["states"] * pset.info["classes"] > 2048 and pset.info["unbounded"] == 0
    assert len(raw_all(native, dec, src, big)) > 100
    small = [b"[a-c]+d", b"e(f|g)*h"]
    found = raw_all(native, dec, src, small)
    want = rows(found, src)
    with rx(native, dec, small) as a, rx(native, dec, small, truth.NO_LDS) as b:
        assert a.info["in_lds"] == 1 and b.info["in_lds"] == 0 and {k: v for k, v in a.info.items() if k != "in_lds"} == {k: v for k, v in b.info.items() if k != "in_lds"}
        raw_search(native, dec, src, b, want)
        raw_grep(dec, src, b, found, False)
        pi = native.PatsetInfo()
        assert native.lib().bzh_patset_get_info(a.handle, native.ctypes.byref(pi)) == 0
        assert (pi.patterns, pi.distinct, pi.min_len, pi.max_len, pi.states, pi.classes, pi.table_bytes) == (
            2, 2, a.info["min_len"], a.info["max_len"], a.info["states"], a.info["classes"], a.info["table_bytes"])
    with native.PatternSet(dec, [b"plain"]) as plain:
        assert native.lib().bzh_regex_get_info(plain.handle, native.ctypes.byref(native.RegexInfo())) == -1


# ---- the full path ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lines(n, seed):
    rng = random.Random(seed)
    vocab = ["".join(rng.choices("etaoinshrdlucmfwypvbgkqjxz", k=rng.randrange(2, 11))) for _ in range(40)]
    src, out, at = " ".join(rng.choices(vocab, k=n // 4)).encode()[:n], bytearray(), 0
    while len(out) < n:
        k = rng.randrange(201) if rng.random() < 0.9 else 0
        out += src[at:at + k] + b"\n"
        at += k
    return bytes(out[:n])


EXPRS = [b"QZ@[A-Za-z]+(#XJ)?", b"[0-9]{4}", b"Err(or)?.*time", b"\nno such line"]
LONG = b"QZ@NeedleInTheHaystack#XJ"


class Input:
    """two streams -- a level-1 one of three blocks and one of one block -- with LONG planted across both block edges and the stream
    edge, at byte 0 and at the last bytes, digits and an "Error ... time" here and there; computed once, never changed"""

    def __init__(self, dec):
        parts = [bytearray(lines(250_000, 31)), bytearray(lines(10_000, 32))]
        pack = lambda: b"".join(bz2.compress(bytes(p), 1 if k == 0 else 9) for k, p in enumerate(parts))
        ent = dec.decode_index(pack())[0]
        assert len(ent) == 4
        bounds = [int(e["out_off"]) for e in ent[1:]]
        whole = bytearray(b"".join(parts))
        self.places = [bounds[0] - 6, bounds[1] - 12, bounds[2] - 12, 0, len(whole) - len(LONG)]
        for at in self.places:
            whole[at:at + len(LONG)] = LONG
        rng = random.Random(33)
        for _ in range(60):
            at = rng.randrange(100, len(whole) - 100)
            if not any(p - 40 < at < p + 40 for p in self.places):
                whole[at:at + 5] = (b"2026 ", b"error", b"ERROR", b"1234567"[:5])[rng.randrange(4)]
        at = 5000  # the first line behind it of 12 to 250 bytes begins with "Error" and ends with "time"
        while not 12 <= whole.index(b"\n", at) - at <= 250:
            at = whole.index(b"\n", at) + 1
        line_end = whole.index(b"\n", at)
        whole[at:at + 5], whole[line_end - 4:line_end] = b"Error", b"time"
        cut = len(parts[0])
        parts = [whole[:cut], whole[cut:]]
        self.s = pack()
        self.truth = bz2.decompress(self.s)
        assert self.truth == bytes(whole)
        self.ent, self.pts, self.cum, self.nrec, total, used = dec.decode_index_records(self.s, 4, 10)
        assert [int(e["out_off"]) for e in self.ent[1:]] == bounds and total == len(whole) and len(self.pts) > 8
        self.bounds = bounds
        self.found = {fold: truth.hits(EXPRS, self.truth, truth.FOLD if fold else 0) for fold in (False, True)}
        self.want = {fold: rows(f, self.truth) for fold, f in self.found.items()}
        for a in (self.ent, self.pts, self.cum):
            a.setflags(write=False)


@pytest.fixture(scope="module")
def inp(dec):
    return Input(dec)


@pytest.mark.parametrize("fold", [False, True])
def test_full_search(dec, inp, native, fold):
    want = inp.want[fold]
    assert {h[0] for h in want if h[2] == 0 and h[3] == len(LONG)} == set(inp.places) and {h[2] for h in want} == {0, 1, 2}
    with rx(native, dec, EXPRS, truth.FOLD if fold else 0) as pset:
        hits, nhits, total, used = dec.search(inp.s, pset, 10, with_total=True)
        assert nhits == len(want) and hit_rows(hits) == want and total == len(inp.truth) and used == len(inp.s)
        ss, ds = dec.search_stats(), dec.decode_stats()
        assert ss["windows"] >= 3 and ss["hits"] == len(want) and ds["blocks"] == 4 and ds["streams"] == 2
        d_in = on_device(inp.s)
        hits, nhits = dec.search_device(d_in.data_ptr(), len(inp.s), pset, 10)
        assert nhits == len(want) and hit_rows(hits) == want
        # max above, at and below the count, and 0
        hits, nhits = dec.search(inp.s, pset, 10, limit=len(want) + 7)
        assert dec.search_status == 0 and nhits == len(want) and hit_rows(hits) == want
        hits, nhits = dec.search(inp.s, pset, 10, limit=len(want))
        assert dec.search_status == 0 and hit_rows(hits) == want
        hits, nhits = dec.search(inp.s, pset, 10, limit=len(want) - 1)
        assert dec.search_status == -4 and nhits == len(want) and hit_rows(hits) == want[:-1]
        hits, nhits = dec.search(inp.s, pset, limit=0)  # the counting call
        assert dec.search_status == 0 and nhits == len(want) and len(hits) == 0


@pytest.mark.parametrize("sync", [False, True])
def test_range_search(dec, inp, native, sync):
    pts = inp.pts if sync else None
    b = inp.bounds
    at0, at1 = inp.places[0], inp.places[1]
    dec.search_set_room(1024)  # every block is a window
    try:
        with rx(native, dec, EXPRS) as pset:
            run = lambda off, length, **kw: dec.search_range(inp.s, inp.ent, pset, off, length, points=pts, rec_cum=inp.cum, delim=10, **kw)
            for off, end in ((0, len(inp.truth)), (b[0] - 5000, b[2] + 5000),
                             (at0, at0 + 10), (at0 - 100, at1 + 8),   # the longest match is cut by the range's end: the longest that fits
                             (at0 + 1, at1 + len(LONG)),              # a match is cut at the start
                             (at1, at1 + 3), (b[2] - 10, len(inp.truth) + 99), (7, 7)):
                want = rows(truth.hits(EXPRS, inp.truth, 0, 256, off, end), inp.truth)
                hits, nhits = run(off, end - off)
                assert nhits == len(want) and hit_rows(hits) == want, (off, end)
            cut = rows(truth.hits(EXPRS, inp.truth, 0, 256, at0 - 100, at1 + 8), inp.truth)
            assert (at0, len(LONG)) in [(h[0], h[3]) for h in cut] and (at1, 8) in [(h[0], h[3]) for h in cut]
            hits, nhits = run(0, None)
            assert hit_rows(hits) == inp.want[False] and dec.search_stats()["windows"] >= 4
            lo, off, end = int(inp.ent[1]["bit_pos"]) // 8, b[0] + 10, b[2] + 10
            hits, nhits = dec.search_range(inp.s[lo:], inp.ent, pset, off, end - off, points=pts, rec_cum=inp.cum, delim=10, in_byte_base=lo)
            assert hit_rows(hits) == rows(truth.hits(EXPRS, inp.truth, 0, 256, off, end), inp.truth)
    finally:
        dec.search_set_room(0)


def test_full_grep_and_index(dec, inp, native):
    for fold in (False, True):
        with rx(native, dec, EXPRS, truth.FOLD if fold else 0) as pset:
            for invert in (False, True):
                want, ent = grep_rows(inp.found[fold], inp.truth, invert)
                data, got = dec.grep(inp.s, pset, b"\n", invert)
                assert data == want and ent_rows(got) == ent, (fold, invert)
                assert dec.grep(inp.s, pset, b"\n", invert, count_only=True) == (len(ent), len(want))
                dec.search_set_room(1024)
                try:
                    for pts in (None, inp.pts):
                        idata, igot = dec.grep_index(inp.s, inp.ent, pset, pts, b"\n", invert)
                        assert idata == want and ent_rows(igot) == ent and dec.grep_stats()["windows"] >= 4
                finally:
                    dec.search_set_room(0)
            want, ent = grep_rows(inp.found[fold], inp.truth)
            d_in, out = on_device(inp.s), room_on_device(len(want))
            for cap, room in ((len(want) - 1, len(ent)), (len(want), len(ent) - 1)):
                st, nrecs, tot, _ = dec.grep_device(d_in.data_ptr(), len(inp.s), pset, out.data_ptr(), cap, room)
                assert (st, nrecs, tot) == (-4, len(ent), len(want)) and "room for" in dec.last_error()
            st, nrecs, tot, got = dec.grep_device(d_in.data_ptr(), len(inp.s), pset, out.data_ptr(), len(want), len(ent))
            host = out.cpu().numpy().tobytes()
            assert (st, nrecs, tot) == (0, len(ent), len(want)) and host[:len(want)] == want and set(host[len(want):]) <= {0xA5} and ent_rows(got) == ent


def test_damaged_input_gives_the_decoders_error(dec, inp, native):
    bad = bytearray(inp.s)
    bad[len(inp.s) // 3] ^= 0x10
    with rx(native, dec, EXPRS) as pset:
        with pytest.raises(native.BzhError) as e1:
            dec.decode(bytes(bad))
        for call in (lambda: dec.search(bytes(bad), pset), lambda: dec.grep(bytes(bad), pset)):
            with pytest.raises(native.BzhError) as e2:
                call()
            assert e1.value.status == e2.value.status == -6 and str(e1.value) == str(e2.value)
        assert dec.search(inp.s, pset)[1] == len(inp.want[False])  # the context and the automaton stay usable


# ---- arguments, Python and the command line -----------------------------------------------------------------------------------------
def test_arguments_and_lifetime(dec, native):
    L, c = native.lib(), native.ctypes
    for exprs, flags, span, text in (([], 0, 0, "0 expressions"), ([b"a", b""], 0, 0, "expression 1, byte 0"), ([b"a"], 8, 0, "flags 0x8"),
                                     ([b"a"], 0, 257, "max_span 257"), ([b"a", b"b*"], 0, 0, "expression 1, byte 0: it matches the empty string"),
                                     ([b"ab^"], 0, 0, "expression 0, byte 2"), ([b"(a|b)*a(a|b){16}"], 0, 0, "states")):
        with pytest.raises(native.BzhError) as err:
            rx(native, dec, exprs, flags, span)
        assert err.value.status == -1 and text in str(err.value), text
    h = c.c_void_p()
    assert L.bzh_regex_create(dec.handle, None, None, 1, 0, 0, c.byref(h)) == -1 and "null" in dec.last_error()
    assert L.bzh_regex_create(dec.handle, None, None, 1, 0, 0, None) == -1
    # destroyed after its context, used with another
    src = text_of(9000, 4)
    want = rows(truth.hits([b"[0-9]+", b"ab+c"], src, truth.FOLD), src)
    first = native.Context(0, 9, 2)
    pset = rx(native, first, [b"[0-9]+", b"ab+c"], truth.FOLD)
    first.close()
    with native.Context(0, 9, 2) as second:
        t = on_device(src)
        hits, nhits = second.search_raw_device(t.data_ptr(), len(src), pset, 10)
        assert nhits == len(want) and hit_rows(hits) == want
    pset.close()
    pset.close()


def test_python_regex(inp):
    import banzai_amd
    with banzai_amd.Regex(EXPRS) as r:
        assert isinstance(r, banzai_amd._native.PatternSet) and r.info["expressions"] == len(EXPRS) and r.info["unbounded"] == 1 and r.info["in_lds"] == 1
        want = inp.want[False]
        hits, nhits = banzai_amd.search(inp.s, r, delim=b"\n")
        assert nhits == len(want) and hit_rows(hits) == want and hits.dtype.names == ("off", "record", "pattern", "len")
        rindex = banzai_amd.build_record_index(inp.s)
        off, end = inp.bounds[0] - 9, inp.bounds[2] + 3
        cut = rows(truth.hits(EXPRS, inp.truth, 0, 256, off, end), inp.truth)
        hits, nhits = banzai_amd.search_range(inp.s, rindex, r, off, end - off)
        assert hit_rows(hits) == cut
        gwant, gent = grep_rows(inp.found[False], inp.truth)
        data, ent = banzai_amd.grep(inp.s, r)
        assert data == gwant and ent_rows(ent) == gent
        assert banzai_amd.grep_count(inp.s, r) == len(gent)
        assert banzai_amd.grep_count(inp.s, r, invert=True, index=rindex.index) == len(grep_rows(inp.found[False], inp.truth, True)[1])
        rd = banzai_amd.IndexedReader(inp.s, rindex)
        hits, nhits = rd.search(r, off, end)
        assert hit_rows(hits) == cut
        assert [k for k, _ in rd.grep(r)] == [e[0] for e in gent] and b"".join(b for _, b in rd.grep(r)) == gwant
    with banzai_amd.Regex(b"err(OR)?", ignore_case=True, max_span=5) as r:
        assert (r.info["min_len"], r.info["max_len"], r.info["unbounded"]) == (3, 5, 0)
        assert [tuple(h)[0::2] for h in hit_rows(banzai_amd.search(inp.s, r)[0])] == [(o, p) for o, p, _ in truth.hits([b"err(OR)?"], inp.truth, truth.FOLD, 5)]
    with banzai_amd.Regex(b"a.b", dotall=True) as r, banzai_amd.Regex(b"a.b") as q:
        both = bz2.compress(b"a\nb a-b\n")
        assert banzai_amd.search(both, r)[1] == 2 and banzai_amd.search(both, q)[1] == 1
    # an escaped word is the word
    word = re.search(rb"[a-z]{5}", inp.truth[7000:]).group(0)
    for w in (word, LONG, b"2026 "):
        with banzai_amd.Regex(re.escape(w)) as r:
            one, n1 = banzai_amd.search(inp.s, w, delim=b"\n")
            many, n2 = banzai_amd.search(inp.s, r, delim=b"\n")
            assert n1 == n2 > 0 and many["off"].tolist() == one["off"].tolist() and many["record"].tolist() == one["record"].tolist()
            assert set(many["len"].tolist()) == {len(w)}


def test_cli(inp, tmp_path):
    exe = os.path.join(ROOT, "banzai_amd", "bnzhip")
    path, pfile = tmp_path / "t.bz2", tmp_path / "exprs.txt"
    path.write_bytes(inp.s)
    run = lambda *args: subprocess.run([exe, *args, str(path)], capture_output=True, timeout=120)
    exprs = [b"qz@[a-z]+#", b"[0-9]{4}"]
    found = truth.hits(exprs, inp.truth, truth.FOLD)
    want, ent = grep_rows(found, inp.truth)
    warn = b"longer than 256 bytes"
    p = run("--grep", exprs[0].decode(), "-e", exprs[1].decode(), "-E", "--ignore-case")
    assert (p.returncode, p.stdout) == (0, want) and warn in p.stderr, p.stderr
    pfile.write_bytes(b"\n".join(exprs) + b"\n")
    p = run("--grep", "--patterns", str(pfile), "--regex", "--ignore-case", "--invert")
    assert (p.returncode, p.stdout) == (0, grep_rows(found, inp.truth, True)[0]), p.stderr
    p = run("--grep", "[0-9]{4}", "-E", "--count")
    cased = truth.hits(exprs[1:], inp.truth)
    assert (p.returncode, p.stdout) == (0, b"%d\n" % len(grep_rows(cased, inp.truth)[1])) and warn not in p.stderr, p.stderr
    p = run("--search", "-e", exprs[0].decode(), "-e", exprs[1].decode(), "-E", "--ignore-case")
    assert (p.returncode, p.stdout) == (0, b"".join(b"%d\t%d\t%d\n" % (o, r, k) for o, r, k, _ in rows(found, inp.truth))), p.stderr
    # without -E the same string is a plain one
    p = run("--grep", "[0-9]{4}", "--count")
    assert (p.returncode, p.stdout) == (0, b"0\n"), p.stderr
    p = run("--grep", "5b302d395d", "-E", "--hex")
    assert p.returncode != 0 and b"--hex" in p.stderr and p.stdout == b""
    p = run("--grep", "a(", "-E")
    assert p.returncode != 0 and b"expression 0, byte 1" in p.stderr
    assert subprocess.run([exe, "-E", str(path)], capture_output=True, timeout=120).returncode != 0
