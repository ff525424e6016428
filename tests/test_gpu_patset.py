"""GPU: search and grep for a SET of patterns in one pass, with ASCII case folding (bzh_patset_*, bzh_search_patset*,
bzh_grep_patset*, banzai_amd.PatternSet, bnzhip -e / --patterns / --ignore-case).  The truth is a bytes.find loop per distinct
pattern -- over bytes.lower() when folding --, sorted by (off, len); for a grep, the records in which such a match starts.  The
context takes batches of 2 candidates, so the blocks of the full input are several batches."""
import bisect
import bz2
import functools
import os
import random
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = (0, 1, 15, 16, 17, 4095, 4096, 4097, 8192, 12289)
LENS = (1, 2, 4, 5, 17, 255, 256)
LONG = b"QZ@Needle#XJ[long]"
SHORT = LONG[:4]


def fold_bytes(b, fold):
    return b.lower() if fold else b  # (bytes.lower folds 'A'..'Z' alone)


def distinct(pats, fold):
    """[(folded pattern, its number)]: of equals the lowest index"""
    seen = {}
    for k, p in enumerate(pats):
        seen.setdefault(fold_bytes(p, fold), k)
    return list(seen.items())


def find_all(t, pat, lo, hi):
    out, at = [], t.find(pat, lo, hi)
    while at >= 0:
        out.append(at)
        at = t.find(pat, at + 1, hi)
    return out


def set_truth(truth, pats, fold, delim=None, lo=0, hi=None):
    """[(off, record, pattern, len)] of the pairs wholly inside [lo, hi), by (off, len)"""
    hi = len(truth) if hi is None else min(hi, len(truth))
    t = fold_bytes(truth, fold)
    rows = [(at, len(f), k) for f, k in distinct(pats, fold) for at in find_all(t, f, lo, hi)]
    rows.sort()
    cuts = np.flatnonzero(np.frombuffer(truth, dtype=np.uint8) == delim) if delim is not None else None
    rec = (lambda at: int(np.searchsorted(cuts, at))) if delim is not None else (lambda at: 0)
    return [(at, rec(at), k, n) for at, n, k in rows]


def grep_truth(truth, pats, fold, delim=b"\n", invert=False):
    """-> (bytes, [(record, off, len, out_off)], nrecords): a record is hit when any pattern's match starts inside it"""
    cut = truth.split(delim)
    recs = [p + delim for p in cut[:-1]] + ([cut[-1]] if cut[-1] else [])
    offs = [0]
    for r in recs:
        offs.append(offs[-1] + len(r))
    hit = {bisect.bisect_right(offs, h[0]) - 1 for h in set_truth(truth, pats, fold)}
    out, ent = bytearray(), []
    for k, r in enumerate(recs):
        if (k in hit) != invert:
            ent.append((k, offs[k], len(r), len(out)))
            out += r
    return bytes(out), ent, len(recs)


def hit_rows(hits):
    return [tuple(int(h[f]) for f in ("off", "record", "pattern", "len")) for h in hits]


def ent_rows(entries):
    return [tuple(int(e[f]) for f in ("record", "off", "len", "out_off")) for e in entries]


@pytest.fixture(scope="module")
def dec(native):
    c = native.Context(0, 9, 2)
    yield c
    c.close()


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


def raw_search(native, dec, src, pats, fold, delim=10):
    want = set_truth(src, pats, fold, delim)
    with native.PatternSet(dec, pats, fold) as pset:
        t = on_device(src)
        st, n0, _ = search_raw_call(native, dec, t, len(src), pset, 1, delim, 0)  # the counting call
        assert (st, n0) == (0, len(want)), (len(src), fold)
        st, n1, hits = search_raw_call(native, dec, t, len(src), pset, 1, delim, len(want))
        assert (st, n1) == (0, len(want)) and hit_rows(hits) == want, (len(src), fold)
        ss = dec.search_stats()
        assert ss["windows"] == 1 and ss["tiles"] == (len(src) + 4095) // 4096 and ss["hits"] == len(want)
    return want


def raw_grep(native, dec, src, pats, fold, invert=False, delim=b"\n"):
    want, ent, nrec = grep_truth(src, pats, fold, delim, invert)
    with native.PatternSet(dec, pats, fold) as pset:
        t = on_device(src)
        st, nrecs, total, _ = dec.grep_raw_device(t.data_ptr(), len(src), pset, 0, 0, 0, delim, invert)  # the counting call
        assert (st, nrecs, total) == (0, len(ent), len(want)), (len(src), fold, invert)
        out = room_on_device(len(want))
        st, nrecs, total, got = dec.grep_raw_device(t.data_ptr(), len(src), pset, out.data_ptr(), len(want), len(ent), delim, invert)
        assert (st, nrecs, total) == (0, len(ent), len(want)), (len(src), fold, invert)
        host = out.cpu().numpy().tobytes()
        assert host[:len(want)] == want and set(host[len(want):]) <= {0xA5}, (len(src), fold, invert)
        assert ent_rows(got) == ent and dec.grep_stats()["records"] == nrec
    return want, ent


def chain(rng, fold):
    """every length a prefix of the next (short and long at one start), a seeded word of every length, the delimiter in a pattern,
    and a pattern given twice"""
    longest = bytes(rng.choice(b"aBcD" if fold else b"abcd") for _ in range(256))
    pats = [longest[:k] for k in LENS] + [bytes(rng.choice(b"abcd") for _ in range(k)) for k in LENS]
    return longest, pats + [b"\n", b"b\n", pats[3]]


# ---- the raw seam ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fold", [False, True])
def test_raw_grid(dec, native, fold):
    rng = random.Random(7 + fold)
    longest, pats = chain(rng, fold)
    found = 0
    for n in NS:
        src = bytes(rng.choice(b"abcdABCD\nx") for _ in range(n))
        found += len(raw_search(native, dec, src, pats, fold))
        raw_grep(native, dec, src, pats, fold)
        raw_grep(native, dec, src, pats, fold, True)
    assert found > 3000


@pytest.mark.parametrize("fold", [False, True])
def test_raw_planted_places(dec, native, fold):
    """offset 0, ending at n - 1, across a thread edge (16), a wave edge (1024) and a tile edge (4096); short and long at one start;
    the longest cut by the text's end while its prefixes still match"""
    rng = random.Random(11 + fold)
    longest, pats = chain(rng, fold)
    for n in (4097, 12289):
        for k in LENS:
            src = bytearray(b"x" * n)
            places, end = [], 0
            for at in sorted({0, n - k, 16 - k // 2, 1024 - k // 2, 4096 - k // 2, 4095, 8192 - k + 1}):
                if 0 <= at and at + k <= n and at >= end:
                    src[at:at + k] = longest[:k]
                    places.append(at)
                    end = at + k
            tail = rng.randrange(1, k + 1)
            src[n - tail:] = longest[:tail]  # (cut by the end of the text)
            for at in range(40, n, 1000):
                src[at] = 10
            src = bytes(src)
            want = raw_search(native, dec, src, pats, fold)
            starts = {h[0] for h in want}
            assert places and all(at in starts for at in places if src[at:at + k] == longest[:k])
            raw_grep(native, dec, src, pats, fold)
    raw_grep(native, dec, src, pats, fold, True)


def test_raw_one_byte_value(dec, native):
    """a text of one byte value and every run of it up to 256 bytes as a pattern: every start holds up to seven hits; every hit slot,
    three, none; the delimiter equal to a pattern byte"""
    pats = [b"z" * k for k in LENS]
    for n in (255, 256, 4097, 12289):
        src = b"z" * n
        want = raw_search(native, dec, src, pats, False, delim=ord("z"))
        assert len(want) == sum(max(0, n - k + 1) for k in LENS)
        with native.PatternSet(dec, pats, True) as pset:
            t = on_device(src.upper())
            st, nh, hits = search_raw_call(native, dec, t, n, pset, 1, ord("Z"), 3)
            assert (st, nh) == (-4, len(want)) and [h[2:] for h in hit_rows(hits)] == [h[2:] for h in want[:3]]
            st, nh, _ = search_raw_call(native, dec, t, n, pset, 0, 0, 0)
            assert (st, nh) == (0, len(want))
        raw_grep(native, dec, src, pats, False, delim=b"z")
        raw_grep(native, dec, src, pats, False, invert=True, delim=b"q")


def test_what_folds(dec, native):
    src = b"@`[{\xc0\xe0aA zZ\n" * 50
    for fold in (False, True):
        pats = [b"@", b"[", b"\xc0", b"A", b"Z\n", b"a", b"z\n"]
        want = raw_search(native, dec, src, pats, fold)
        assert len(want) == 300 and not {h[0] % 12 for h in want} & {1, 3, 5}  # ('`', '{' and 0xE0 match nothing, folded or not)
        with native.PatternSet(dec, pats, fold) as pset:
            assert pset.info["distinct"] == (5 if fold else 7) and pset.info["patterns"] == 7
            assert pset.info["min_len"] == 1 and pset.info["max_len"] == 2 and pset.info["table_bytes"] == 2 * pset.info["states"] * pset.info["classes"]


# ---- equivalence with the single-pattern calls --------------------------------------------------------------------------------------
def test_a_set_of_one_is_the_single_pattern(dec, native):
    rng = random.Random(3)
    src = bytes(rng.choice(b"ab\nc\n") for _ in range(12289))
    t = on_device(src)
    for plen in (1, 3, 5, 17, 256):
        at = rng.randrange(len(src) - plen)
        pat = src[at:at + plen]
        one, n1 = dec.search_raw_device(t.data_ptr(), len(src), pat, 10)
        with native.PatternSet(dec, [pat]) as pset:
            many, n2 = dec.search_raw_device(t.data_ptr(), len(src), pset, 10)
            assert n1 == n2 and n1 > 0
            assert many["off"].tolist() == one["off"].tolist() and many["record"].tolist() == one["record"].tolist()
            assert set(many["pattern"].tolist()) == {0} and set(many["len"].tolist()) == {plen}
            for invert in (False, True):
                st, nrecs, total, _ = dec.grep_raw_device(t.data_ptr(), len(src), pat, 0, 0, 0, b"\n", invert)
                o1, o2 = room_on_device(total), room_on_device(total)
                r1 = dec.grep_raw_device(t.data_ptr(), len(src), pat, o1.data_ptr(), total, nrecs, b"\n", invert)
                r2 = dec.grep_raw_device(t.data_ptr(), len(src), pset, o2.data_ptr(), total, nrecs, b"\n", invert)
                assert r1[:3] == r2[:3] == (0, nrecs, total) and ent_rows(r1[3]) == ent_rows(r2[3])
                assert o1.cpu().numpy().tobytes() == o2.cpu().numpy().tobytes()


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


class Input:
    """three streams -- a level-1 one of three blocks, two of one block -- with LONG (and so SHORT, its first four bytes) planted
    across every block boundary, the batch boundary and both stream boundaries among them, at byte 0 and at the last bytes, in
    changing case; computed once, never changed"""

    def __init__(self, dec):
        parts = [bytearray(lines(250_000, 21)), bytearray(lines(10_000, 22)), bytearray(lines(10_000, 23))]
        pack = lambda: b"".join(bz2.compress(bytes(p), 1 if k == 0 else 9) for k, p in enumerate(parts))
        ent = dec.decode_index(pack())[0]
        assert len(ent) == 5
        bounds = [int(e["out_off"]) for e in ent[1:]]
        whole = bytearray(b"".join(parts))
        half = len(LONG) // 2
        # (at b - 6 SHORT ends in front of the boundary and LONG, at the same start, spans it)
        self.places = [bounds[0] - 6, bounds[1] - 6, bounds[2] - half, bounds[3] - half, 0, len(whole) - len(LONG)]
        for j, at in enumerate(self.places):
            whole[at:at + len(LONG)] = (LONG, LONG.upper(), LONG.lower())[j % 3]
        cuts = [0, len(parts[0]), len(parts[0]) + len(parts[1]), len(whole)]
        parts = [whole[cuts[k]:cuts[k + 1]] for k in range(3)]
        self.s = pack()
        self.truth = bz2.decompress(self.s)
        assert self.truth == bytes(whole)
        self.ent, self.pts, self.cum, self.nrec, total, used = dec.decode_index_records(self.s, 4, 10)
        assert [int(e["out_off"]) for e in self.ent[1:]] == bounds and total == len(whole) and len(self.pts) > 8
        self.bounds = bounds
        self.word = re.search(rb"[a-z]{4}", self.truth[5000:]).group(0)
        self.pats = [LONG, SHORT, b"#XJ", self.word, LONG.upper(), b"\nno such line"]
        for a in (self.ent, self.pts, self.cum):
            a.setflags(write=False)


@pytest.fixture(scope="module")
def inp(dec):
    return Input(dec)


@pytest.mark.parametrize("fold", [False, True])
def test_full_search(dec, inp, native, fold):
    want = set_truth(inp.truth, inp.pats, fold, 10)
    assert {h[0] for h in want if h[3] == len(LONG)} == set(inp.places if fold else inp.places[0:2] + inp.places[3:5])
    with native.PatternSet(dec, inp.pats, fold) as pset:
        hits, nhits, total, used = dec.search(inp.s, pset, 10, with_total=True)
        assert nhits == len(want) and hit_rows(hits) == want and total == len(inp.truth) and used == len(inp.s)
        ss, ds = dec.search_stats(), dec.decode_stats()
        assert ss["windows"] >= 4 and ss["hits"] == len(want) and ds["blocks"] == 5 and ds["streams"] == 3  # (one window finishes the carry)
        d_in = on_device(inp.s)
        hits, nhits = dec.search_device(d_in.data_ptr(), len(inp.s), pset, 10)
        assert nhits == len(want) and hit_rows(hits) == want
        # rooms: one below the need is BZH_E_CAP with the exact total and the first hits; the repeat succeeds
        hits, nhits = dec.search(inp.s, pset, 10, limit=len(want) - 1)
        assert dec.search_status == -4 and nhits == len(want) and hit_rows(hits) == want[:-1]
        hits, nhits = dec.search(inp.s, pset, 10, limit=len(want))
        assert dec.search_status == 0 and hit_rows(hits) == want
        hits, nhits = dec.search(inp.s, pset, limit=0)  # the counting call
        assert dec.search_status == 0 and nhits == len(want) and len(hits) == 0


@pytest.mark.parametrize("sync", [False, True])
def test_range_search(dec, inp, native, sync):
    pts = inp.pts if sync else None
    b = inp.bounds
    at0, at1 = inp.places[0], inp.places[1]
    dec.search_set_room(1024)  # every block is a window
    try:
        for fold in (False, True):
            with native.PatternSet(dec, inp.pats, fold) as pset:
                run = lambda off, length, **kw: dec.search_range(inp.s, inp.ent, pset, off, length, points=pts, rec_cum=inp.cum, delim=10, **kw)
                for off, end in ((0, len(inp.truth)), (b[0] - 5000, b[2] + 5000),
                                 (at0, at0 + 10), (at0 - 100, at1 + 6),   # the long pattern is cut at the end, its short prefix is kept
                                 (at0 + 1, at1 + len(LONG)),              # a match is cut at the start
                                 (at1, at1 + 3), (b[3] - 10, len(inp.truth) + 99), (7, 7)):
                    want = set_truth(inp.truth, inp.pats, fold, 10, off, end)
                    hits, nhits = run(off, end - off)
                    assert nhits == len(want) and hit_rows(hits) == want, (off, end, fold)
                want = set_truth(inp.truth, inp.pats, fold, 10)
                hits, nhits = run(0, None)
                assert hit_rows(hits) == want and dec.search_stats()["windows"] >= 5
                lo, hi = int(inp.ent[1]["bit_pos"]) // 8, len(inp.s)
                off, end = b[0] + 10, b[3] + 10
                hits, nhits = dec.search_range(inp.s[lo:hi], inp.ent, pset, off, end - off, points=pts, rec_cum=inp.cum, delim=10, in_byte_base=lo)
                assert hit_rows(hits) == set_truth(inp.truth, inp.pats, fold, 10, off, end)
                d_in = on_device(inp.s)
                hits, nhits = dec.search_range(len(inp.s), inp.ent, pset, off, end - off, points=pts, d_in=d_in.data_ptr())  # no record table
                assert [(h[0], h[2], h[3]) for h in hit_rows(hits)] == [(h[0], h[2], h[3]) for h in set_truth(inp.truth, inp.pats, fold, None, off, end)]
    finally:
        dec.search_set_room(0)


def test_full_grep_and_index(dec, inp, native):
    for fold in (False, True):
        with native.PatternSet(dec, inp.pats, fold) as pset:
            for invert in (False, True):
                want, ent, nrec = grep_truth(inp.truth, inp.pats, fold, b"\n", invert)
                data, got = dec.grep(inp.s, pset, b"\n", invert)
                assert data == want and ent_rows(got) == ent and dec.grep_stats()["records"] == nrec, (fold, invert)
                assert dec.grep(inp.s, pset, b"\n", invert, count_only=True) == (len(ent), len(want))
                dec.search_set_room(1024)
                try:
                    for pts in (None, inp.pts):
                        idata, igot = dec.grep_index(inp.s, inp.ent, pset, pts, b"\n", invert)
                        assert idata == want and ent_rows(igot) == ent and dec.grep_stats()["windows"] >= 5
                finally:
                    dec.search_set_room(0)
            want, ent, _ = grep_truth(inp.truth, inp.pats, fold)
            d_in, out = on_device(inp.s), room_on_device(len(want))
            for cap, room in ((len(want) - 1, len(ent)), (len(want), len(ent) - 1)):
                st, nrecs, tot, _ = dec.grep_device(d_in.data_ptr(), len(inp.s), pset, out.data_ptr(), cap, room)
                assert (st, nrecs, tot) == (-4, len(ent), len(want)) and "room for" in dec.last_error()
            st, nrecs, tot, got = dec.grep_device(d_in.data_ptr(), len(inp.s), pset, out.data_ptr(), len(want), len(ent))
            host = out.cpu().numpy().tobytes()
            assert (st, nrecs, tot) == (0, len(ent), len(want)) and host[:len(want)] == want and set(host[len(want):]) <= {0xA5} and ent_rows(got) == ent
            st, nrecs, tot, got = dec.grep_index_device(d_in.data_ptr(), len(inp.s), inp.ent, pset, out.data_ptr(), len(want), len(ent), inp.pts)
            assert (st, nrecs, tot) == (0, len(ent), len(want)) and out.cpu().numpy().tobytes()[:len(want)] == want and ent_rows(got) == ent


def test_damaged_input_gives_the_decoders_error(dec, inp, native):
    bad = bytearray(inp.s)
    bad[len(inp.s) // 3] ^= 0x10
    with native.PatternSet(dec, inp.pats) as pset:
        with pytest.raises(native.BzhError) as e1:
            dec.decode(bytes(bad))
        for call in (lambda: dec.search(bytes(bad), pset), lambda: dec.grep(bytes(bad), pset)):
            with pytest.raises(native.BzhError) as e2:
                call()
            assert e1.value.status == e2.value.status == -6 and str(e1.value) == str(e2.value)
        assert dec.search(inp.s, pset)[1] == len(set_truth(inp.truth, inp.pats, False))  # the context and the set stay usable


# ---- arguments ---------------------------------------------------------------------------------------------------------------------
def test_arguments(dec, native):
    L, c = native.lib(), native.ctypes
    make = lambda pats, flags=0: native.PatternSet(dec, pats, flags=flags)
    for pats, flags, text in (([], 0, "0 patterns"), ([b"a", b""], 0, "pattern 1 has 0 bytes"), ([b"a", b"b", b"x" * 257], 0, "pattern 2 has 257 bytes"),
                              ([b"a"], 2, "flags 0x2"), ([b"a"] * 65537, 0, "65537 patterns")):
        with pytest.raises(native.BzhError) as err:
            make(pats, flags)
        assert err.value.status == -1 and text in str(err.value), text
    rng = random.Random(1)
    many = [bytes(rng.randrange(256) for _ in range(256)) for _ in range(300)]  # above 65,535 states
    with pytest.raises(native.BzhError) as err:
        make(many)
    assert err.value.status == -1 and "states" in str(err.value) and any(ch.isdigit() for ch in str(err.value))
    h = c.c_void_p()
    assert L.bzh_patset_create(dec.handle, None, None, 1, 0, c.byref(h)) == -1 and "null" in dec.last_error()
    assert L.bzh_patset_create(dec.handle, None, None, 1, 0, None) == -1
    src = lines(9000, 6)
    t = on_device(src)
    got, total = c.c_size_t(0), c.c_uint64(0)
    with make([b"e", b"sh"]) as pset:
        args = (dec.handle, t.data_ptr(), len(src))
        assert L.bzh_search_patset_raw_device(*args, None, 0, 10, None, 0, c.byref(got)) == -1  # no set
        assert L.bzh_search_patset_raw_device(*args, pset.handle, 2, 10, None, 0, c.byref(got)) == -1 and "BZH_SEARCH_RECORDS" in dec.last_error()
        assert L.bzh_search_patset_raw_device(*args, pset.handle, 0, 10, None, 4, c.byref(got)) == -1  # a null array with room claimed
        assert L.bzh_search_patset_raw_device(*args, pset.handle, 0, 10, None, 0, None) == -1
        assert L.bzh_search_patset_raw_device(dec.handle, t.data_ptr() + 1, len(src) - 1, pset.handle, 0, 10, None, 0, c.byref(got)) == -1
        assert "16-byte aligned" in dec.last_error()
        assert L.bzh_grep_patset_raw_device(*args, None, 0, 10, None, 0, None, 0, c.byref(got), c.byref(total)) == -1
        assert L.bzh_grep_patset_raw_device(*args, pset.handle, 2, 10, None, 0, None, 0, c.byref(got), c.byref(total)) == -1
        assert L.bzh_grep_patset_raw_device(*args, pset.handle, 0, 10, None, 4, None, 0, c.byref(got), c.byref(total)) == -1
        assert L.bzh_grep_patset_raw_device(*args, pset.handle, 0, 10, None, 0, None, 0, None, c.byref(total)) == -1
        # rooms one below the need: BZH_E_CAP with the exact totals, and the repeat succeeds
        want = set_truth(src, [b"e", b"sh"], False, 10)
        st, nh, hits = search_raw_call(native, dec, t, len(src), pset, 1, 10, len(want) - 1)
        assert (st, nh) == (-4, len(want)) and hit_rows(hits) == want[:-1] and "room for" in dec.last_error()
        st, nh, hits = search_raw_call(native, dec, t, len(src), pset, 1, 10, len(want))
        assert (st, nh) == (0, len(want)) and hit_rows(hits) == want
        gwant, gent, _ = grep_truth(src, [b"e", b"sh"], False)
        out = room_on_device(len(gwant))
        for cap, room in ((len(gwant) - 1, len(gent)), (len(gwant), len(gent) - 1)):
            st, nrecs, tot, _ = dec.grep_raw_device(t.data_ptr(), len(src), pset, out.data_ptr(), cap, room)
            assert (st, nrecs, tot) == (-4, len(gent), len(gwant))
        st, nrecs, tot, ge = dec.grep_raw_device(t.data_ptr(), len(src), pset, out.data_ptr(), len(gwant), len(gent))
        assert (st, nrecs, tot) == (0, len(gent), len(gwant)) and ent_rows(ge) == gent


def test_a_set_outlives_its_context(native):
    src = lines(9000, 6)
    pats = [b"e", b"SH", b"the"]
    want = set_truth(src, pats, True, 10)
    first = native.Context(0, 9, 2)
    pset = native.PatternSet(first, pats, True)
    first.close()
    with native.Context(0, 9, 2) as second:
        t = on_device(src)
        hits, nhits = second.search_raw_device(t.data_ptr(), len(src), pset, 10)
        assert nhits == len(want) and hit_rows(hits) == want
    pset.close()
    pset.close()


def test_a_set_of_another_device(native):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device is visible: a set of another device cannot be made")
    with native.Context(0, 9, 2) as c0, native.Context(1, 9, 2) as c1, native.PatternSet(c1, [b"e"]) as pset:
        t = on_device(b"seven")
        with pytest.raises(native.BzhError) as err:
            c0.search_raw_device(t.data_ptr(), 5, pset)
        assert err.value.status == -1 and "device" in str(err.value)


# ---- Python and the command line ------------------------------------------------------------------------------------------------------
def test_python_pattern_set(inp):
    import banzai_amd
    for fold in (False, True):
        with banzai_amd.PatternSet(inp.pats, ignore_case=fold) as pset:
            assert pset.info["patterns"] == len(inp.pats) and pset.info["distinct"] == (5 if fold else 6)
            want = set_truth(inp.truth, inp.pats, fold, 10)
            hits, nhits = banzai_amd.search(inp.s, pset, delim=b"\n")
            assert nhits == len(want) and hit_rows(hits) == want and hits.dtype.names == ("off", "record", "pattern", "len")
            rindex = banzai_amd.build_record_index(inp.s)
            off, end = inp.bounds[0] - 9, inp.bounds[2] + 3
            hits, nhits = banzai_amd.search_range(inp.s, rindex, pset, off, end - off)
            assert hit_rows(hits) == set_truth(inp.truth, inp.pats, fold, 10, off, end)
            gwant, gent, _ = grep_truth(inp.truth, inp.pats, fold)
            data, ent = banzai_amd.grep(inp.s, pset)
            assert data == gwant and ent_rows(ent) == gent
            assert banzai_amd.grep_count(inp.s, pset) == len(gent)
            assert banzai_amd.grep_count(inp.s, pset, invert=True, index=rindex.index) == len(grep_truth(inp.truth, inp.pats, fold, invert=True)[1])
            rd = banzai_amd.IndexedReader(inp.s, rindex)
            hits, nhits = rd.search(pset, off, end)
            assert hit_rows(hits) == set_truth(inp.truth, inp.pats, fold, 10, off, end)
            assert [r for r, _ in rd.grep(pset)] == [e[0] for e in gent] and b"".join(b for _, b in rd.grep(pset)) == gwant
    # bytes go the way they went
    hits, nhits = banzai_amd.search(inp.s, LONG, delim=b"\n")
    assert hits.dtype.names == ("off", "record") and nhits == 2


def test_cli(inp, tmp_path):
    exe = os.path.join(ROOT, "banzai_amd", "bnzhip")
    path, pfile = tmp_path / "t.bz2", tmp_path / "pats.txt"
    path.write_bytes(inp.s)
    run = lambda *args: subprocess.run([exe, *args, str(path)], capture_output=True, timeout=120)
    A, Bw = inp.word.decode(), "qz@n"
    pats = [A.encode(), Bw.encode()]
    want, ent, nrec = grep_truth(inp.truth, pats, True)
    p = run("--grep", "-e", A, "-e", Bw, "--ignore-case")
    assert (p.returncode, p.stdout) == (0, want), p.stderr
    p = run("--grep", A.encode().hex(), "-e", Bw.encode().hex(), "--ignore-case", "--hex")
    assert (p.returncode, p.stdout) == (0, want), p.stderr
    pfile.write_bytes(b"\n".join(pats) + b"\n")
    p = run("--grep", "--patterns", str(pfile), "--ignore-case")
    assert (p.returncode, p.stdout) == (0, want), p.stderr
    inv, ient, _ = grep_truth(inp.truth, pats, True, invert=True)
    p = run("--grep", "--patterns", str(pfile), "--ignore-case", "--invert")
    assert (p.returncode, p.stdout) == (0, inv) and len(ent) + len(ient) == nrec, p.stderr
    p = run("--grep", "-e", A, "-e", Bw, "--count")
    assert (p.returncode, p.stdout) == (0, b"%d\n" % len(grep_truth(inp.truth, pats, False)[1])), p.stderr
    p = run("--search", "-e", LONG.decode(), "-e", SHORT.decode(), "-e", A)
    hits = set_truth(inp.truth, [LONG, SHORT, A.encode()], False, 10)
    assert (p.returncode, p.stdout) == (0, b"".join(b"%d\t%d\t%d\n" % (o, r, k) for o, r, k, _ in hits)), p.stderr
    p = run("--search", SHORT.decode(), "--ignore-case", "--count")
    assert (p.returncode, p.stdout) == (0, b"%d\n" % len(set_truth(inp.truth, [SHORT], True))), p.stderr
    pfile.write_bytes(b"one\n\nthree\n")
    p = run("--grep", "--patterns", str(pfile))
    assert p.returncode != 0 and b"line 2" in p.stderr
    assert run("--grep", "-e").returncode != 0 and run("-e", A).returncode != 0
    # one plain string goes the way it went: the single-pattern call's bytes
    import banzai_amd
    p = run("--grep", A)
    assert (p.returncode, p.stdout) == (0, banzai_amd.grep(inp.s, A.encode())[0]), p.stderr
    p = run("--search", A)
    one = banzai_amd.search(inp.s, A.encode(), delim=b"\n")[0]
    assert (p.returncode, p.stdout) == (0, b"".join(b"%d\t%d\n" % (int(h["off"]), int(h["record"])) for h in one)), p.stderr
