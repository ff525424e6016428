"""GPU: grep inside decoded bytes that stay on the device (bzh_grep_raw_device, bzh_grep*, bzh_grep_index*, banzai_amd.grep /
grep_count, bnzhip --grep).  The truth is always bz2.decompress(stream) cut with split(delim); a record is hit when a match STARTS
inside it -- "a match that spans a delimiter belongs to the record of its first byte" --, which for a pattern without the delimiter
is `pattern in record`.  The context takes batches of 2 candidates, so the five blocks of the input are several batches; one block
holds no delimiter, so a record runs across two batch edges."""
import bisect
import bz2
import functools
import os
import random
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = (0, 1, 15, 16, 17, 4095, 4096, 4097, 8192, 12289)
PLENS = (1, 2, 3, 4, 5, 16, 17, 255, 256)
NEEDLE = b"QZ@needle#XJ"
CARRIED = b"only-in-the-carry"


@functools.lru_cache(maxsize=None)
def text(n, seed, words=40):
    rng = random.Random(seed)
    vocab = ["".join(rng.choices("etaoinshrdlucmfwypvbgkqjxz", k=rng.randrange(2, 11))) for _ in range(words)]
    return " ".join(rng.choices(vocab, k=n // 4)).encode()[:n]


@functools.lru_cache(maxsize=None)
def lines(n, seed):
    """the same text cut into lines of 0 to 200 bytes"""
    rng = random.Random(seed)
    src, out, at = text(n, seed), bytearray(), 0
    while len(out) < n:
        k = rng.randrange(201) if rng.random() < 0.9 else 0
        out += src[at:at + k] + b"\n"
        at += k
    return bytes(out[:n])


def find_all(truth, pat):
    out, at = [], truth.find(pat)
    while at >= 0:
        out.append(at)
        at = truth.find(pat, at + 1)
    return out


def grep_truth(truth, pat, delim=b"\n", invert=False):
    """-> (bytes, [(record, off, len, out_off)], nrecords)"""
    cut = truth.split(delim)
    recs = [p + delim for p in cut[:-1]] + ([cut[-1]] if cut[-1] else [])  # (an empty tail is not a record)
    offs = [0]
    for r in recs:
        offs.append(offs[-1] + len(r))
    hit = {bisect.bisect_right(offs, s) - 1 for s in find_all(truth, pat)}  # the record of the match's first byte
    if delim not in pat:
        assert hit == {k for k, r in enumerate(recs) if pat in r}
    out, ent = bytearray(), []
    for k, r in enumerate(recs):
        if (k in hit) != invert:
            ent.append((k, offs[k], len(r), len(out)))
            out += r
    return bytes(out), ent, len(recs)


def rows(entries):
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


def raw(dec, src, pat, invert=False, delim=b"\n"):
    """bzh_grep_raw_device with the exact rooms, checked against the truth; nothing behind the room is touched"""
    want, ent, nrec = grep_truth(src, pat, delim, invert)
    t = on_device(src)
    assert t.data_ptr() % 16 == 0
    st, nrecs, total, _ = dec.grep_raw_device(t.data_ptr(), len(src), pat, 0, 0, 0, delim, invert)  # the counting call
    assert (st, nrecs, total) == (0, len(ent), len(want)), (len(src), pat[:20], invert)
    out = room_on_device(len(want))
    st, nrecs, total, got = dec.grep_raw_device(t.data_ptr(), len(src), pat, out.data_ptr(), len(want), len(ent), delim, invert)
    assert (st, nrecs, total) == (0, len(ent), len(want)), (len(src), pat[:20], invert)
    host = out.cpu().numpy().tobytes()
    assert host[:len(want)] == want and set(host[len(want):]) <= {0xA5}, (len(src), pat[:20], invert)
    assert rows(got) == ent, (len(src), pat[:20], invert)
    assert dec.grep_stats()["records"] == nrec
    return want, ent


# ---- the raw seam: the kernels on a device buffer ---------------------------------------------------------------------------
def test_raw_grid(dec):
    rng = random.Random(5)
    for n in NS:
        src = bytes(rng.choice(b"ab\nc\n") for _ in range(n))
        for plen in PLENS:
            pat = bytes(rng.choice(b"ab") for _ in range(plen))
            if n >= plen and rng.random() < 0.8:
                at = rng.randrange(n - plen + 1)
                pat = src[at:at + plen]  # (the delimiter is a pattern byte, often)
            for invert in (False, True):
                raw(dec, src, pat, invert)
        st = dec.grep_stats()
        assert st["windows"] == 1 and st["tiles"] == (n + 4095) // 4096


def test_raw_fixed_places(dec):
    n = 12289
    for plen in (1, 5, 17, 256):
        pat = bytes(65 + j % 23 for j in range(plen))
        # a delimiter as the last byte of a thread, a wave and a tile, and as the first byte of the next
        src = bytearray(b"x" * n)
        for at in (15, 16, 1023, 1024, 4095, 4096, 8191):
            src[at] = 10
        src[2000:2000 + plen] = pat
        src[n - plen:] = pat
        for invert in (False, True):
            raw(dec, bytes(src), pat, invert)
        # a record over three tiles with its only hit in the first, the middle and the last tile
        for at in (300, 5000, 9000):
            src = bytearray(b"c" * n)
            src[100] = src[101] = src[12000] = 10
            src[at:at + plen] = pat
            want, ent = raw(dec, bytes(src), pat)
            assert [e[0] for e in ent] == [2] and ent[0][2] == 12000 - 101
            raw(dec, bytes(src), pat, True)
    # delimiters only, no delimiter, the pattern is the delimiter, begins with it, ends with it
    raw(dec, b"\n" * n, b"a")
    raw(dec, b"\n" * n, b"\n")
    raw(dec, b"\n" * n, b"\n\n\n", True)
    raw(dec, b"ab" * 3000, b"ba")
    raw(dec, b"ab" * 3000, b"bb", True)
    src = lines(n, 3)
    for pat in (b"\n", b"\ne", b"e\n", b"\n\n"):
        for invert in (False, True):
            raw(dec, src, pat, invert)
    # selected output that starts at every residue modulo 16
    for first in range(1, 17):
        src = b"c" * (first - 1) + b"\n" + lines(5000, 4)
        raw(dec, src, b"e", True)
        raw(dec, src, b"\n" if first == 1 else b"c")
    assert dec.grep_raw_device(0, 0, b"a", 0, 0, 0)[:3] == (0, 0, 0)


def test_raw_more_tiles_than_scan_threads(dec):
    """700 and 2,400 tiles: every thread of grep_scan walks a run of tiles, in batches of eight and a rest"""
    base = lines(200_000, 7)
    for tiles in (700, 2400):
        n = tiles * 4096 + 77
        src = bytearray((base * (n // len(base) + 1))[:n])
        for at in range(5000, n - len(NEEDLE), 700_001):
            src[at:at + len(NEEDLE)] = NEEDLE
        src = bytes(src)
        want, ent = raw(dec, src, NEEDLE)
        assert len(ent) >= n // 700_001 and dec.grep_stats()["tiles"] == tiles + 1
        raw(dec, src, NEEDLE, True)
        raw(dec, src, base[5000:5004])


def test_raw_arguments_and_rooms(dec, native):
    src = lines(9000, 6)
    t = on_device(src)
    want, ent, _ = grep_truth(src, b"e")
    assert len(ent) > 10
    out = room_on_device(len(want))
    for bad in (b"", b"a" * 257):
        assert dec.grep_raw_device(t.data_ptr(), len(src), bad, 0, 0, 0)[0] == -1
    assert dec.grep_raw_device(t.data_ptr() + 1, len(src) - 1, b"e", 0, 0, 0)[0] == -1 and "16-byte aligned" in dec.last_error()
    assert dec.grep_raw_device(t.data_ptr(), len(src), b"e", out.data_ptr() + 2, 10, 0)[0] == -1 and "4-byte aligned" in dec.last_error()
    assert dec.grep_raw_device(t.data_ptr(), len(src), b"e", 0, 0, 0, flags=2)[0] == -1
    L, c = native.lib(), native.ctypes
    pat = np.frombuffer(b"e", dtype=np.uint8)
    got, total = c.c_size_t(0), c.c_uint64(0)
    args = (dec.handle, t.data_ptr(), len(src), native.ptr(pat), 1, 0, 10)
    assert L.bzh_grep_raw_device(*args, None, 4, None, 0, c.byref(got), c.byref(total)) == -1  # a null array with room claimed
    assert L.bzh_grep_raw_device(*args, None, 0, None, 4, c.byref(got), c.byref(total)) == -1
    assert L.bzh_grep_raw_device(*args, None, 0, None, 0, None, c.byref(total)) == -1
    assert L.bzh_grep_raw_device(*args, None, 0, None, 0, c.byref(got), None) == -1
    assert L.bzh_grep_raw_device(dec.handle, t.data_ptr(), len(src), None, 1, 0, 10, None, 0, None, 0, c.byref(got), c.byref(total)) == -1
    # rooms: one below the need is BZH_E_CAP with the exact totals; an array that is not asked for never is
    for cap, room in ((len(want) - 1, len(ent)), (len(want), len(ent) - 1)):
        st, nrecs, tot, _ = dec.grep_raw_device(t.data_ptr(), len(src), b"e", out.data_ptr(), cap, room)
        assert (st, nrecs, tot) == (-4, len(ent), len(want))
    st, nrecs, tot, got_ent = dec.grep_raw_device(t.data_ptr(), len(src), b"e", 0, 0, len(ent))  # entries alone
    assert (st, nrecs, tot) == (0, len(ent), len(want)) and rows(got_ent) == ent
    st, nrecs, tot, _ = dec.grep_raw_device(t.data_ptr(), len(src), b"e", out.data_ptr(), len(want), 0)  # bytes alone
    assert (st, nrecs, tot) == (0, len(ent), len(want)) and out.cpu().numpy().tobytes()[:len(want)] == want


# ---- the full call ------------------------------------------------------------------------------------------------------------
class Input:
    """three streams -- a level-1 one of three blocks, two of one block -- with NEEDLE planted across every block boundary (the
    batch boundary and both stream boundaries among them), at byte 0 and at the last byte; block 2 holds no delimiter, so one
    record begins in block 1, runs across two batch edges and ends in block 3, and CARRIED lies only in its part inside block 1;
    computed once, never changed"""

    def __init__(self, dec):
        parts = [bytearray(lines(250_000, 11)), bytearray(lines(10_000, 12)), bytearray(lines(10_000, 13))]
        pack = lambda: b"".join(bz2.compress(bytes(p), 1 if k == 0 else 9) for k, p in enumerate(parts))
        ent = dec.decode_index(pack())[0]
        assert len(ent) == 5
        bounds = [int(e["out_off"]) for e in ent[1:]]
        whole = bytearray(b"".join(parts))
        lo, hi = bounds[0] - 700, bounds[1] + 300
        whole[lo:hi] = bytes(whole[lo:hi]).replace(b"\n", b"_")  # (the runs keep their lengths: the blocks keep their bounds)
        half = len(NEEDLE) // 2
        for at in [0, len(whole) - len(NEEDLE)] + [b - half for b in bounds]:
            whole[at:at + len(NEEDLE)] = NEEDLE
        whole[lo + 100:lo + 100 + len(CARRIED)] = CARRIED
        cuts = [0, len(parts[0]), len(parts[0]) + len(parts[1]), len(whole)]
        parts = [whole[cuts[k]:cuts[k + 1]] for k in range(3)]
        self.s = pack()
        self.truth = bz2.decompress(self.s)
        assert self.truth == bytes(whole)
        self.ent, self.pts, total, used = dec.decode_index_sync(self.s, 4)
        assert [int(e["out_off"]) for e in self.ent[1:]] == bounds and total == len(whole) and len(self.pts) > 8
        self.bounds = bounds
        self.long = (lo, hi)
        for a in (self.ent, self.pts):
            a.setflags(write=False)


@pytest.fixture(scope="module")
def inp(dec):
    return Input(dec)


def full(dec, inp, pat, invert=False):
    want, ent, nrec = grep_truth(inp.truth, pat, b"\n", invert)
    data, got = dec.grep(inp.s, pat, b"\n", invert)
    assert data == want and rows(got) == ent, (pat[:20], invert)
    assert dec.grep_stats()["records"] == nrec
    return want, ent


def test_full_grep_across_every_boundary(dec, inp):
    want, ent = full(dec, inp, NEEDLE)
    assert len(ent) == 5 and ent[0][0] == 0 and ent[-1][1] + ent[-1][2] == len(inp.truth)  # (two of the six lie in the long record)
    st, ds = dec.grep_stats(), dec.decode_stats()
    assert st["windows"] >= 3 and st["carry_peak"] > 512  # the edges were reached
    assert st["selected"] == 5 and st["out_bytes"] == len(want) and ds["blocks"] == 5 and ds["streams"] == 3
    # the hit lies only in the carried part of the long record
    want, ent = full(dec, inp, CARRIED)
    assert len(ent) == 1 and ent[0][1] < inp.bounds[0] and ent[0][1] + ent[0][2] > inp.bounds[1] and ent[0][2] > 50_000
    # words on many lines, one byte, a newline in the pattern, and each inverted
    for pat in (inp.truth[5000:5003], b"e", b"\n", b"e\n", b"\n" + inp.truth[5000:5001], inp.truth[inp.bounds[2] - 100:inp.bounds[2] + 100]):
        full(dec, inp, pat)
        full(dec, inp, pat, True)
    full(dec, inp, b"no such bytes anywhere")
    assert len(full(dec, inp, b"no such bytes anywhere", True)[0]) == len(inp.truth)


def test_full_grep_rooms_and_the_device_variant(dec, inp, native):
    pat = inp.truth[5000:5003]
    want, ent, _ = grep_truth(inp.truth, pat)
    assert len(ent) > 100
    assert dec.grep(inp.s, pat, count_only=True) == (len(ent), len(want))
    d_in, out = on_device(inp.s), room_on_device(len(want))
    for cap, room in ((len(want) - 1, len(ent)), (len(want), len(ent) - 1)):
        st, nrecs, tot, _ = dec.grep_device(d_in.data_ptr(), len(inp.s), pat, out.data_ptr(), cap, room)
        assert (st, nrecs, tot) == (-4, len(ent), len(want)) and "room for" in dec.last_error()
    st, nrecs, tot, got = dec.grep_device(d_in.data_ptr(), len(inp.s), pat, out.data_ptr(), len(want), len(ent))
    host = out.cpu().numpy().tobytes()
    assert (st, nrecs, tot) == (0, len(ent), len(want)) and host[:len(want)] == want and set(host[len(want):]) <= {0xA5} and rows(got) == ent
    assert dec.grep(inp.s, pat)[0] == want  # the host variant gives the same bytes


def test_full_grep_errors_are_the_decoders(dec, inp, native):
    bad = bytearray(inp.s)
    bad[len(inp.s) // 3] ^= 0x10  # a damaged block
    crc = bytearray(inp.s)
    crc[-3] ^= 0x10  # the last stream's CRC (its 32 bits end within the last byte)
    for broken in (bytes(bad), bytes(crc)):
        with pytest.raises(native.BzhError) as e1:
            dec.decode(broken)
        with pytest.raises(native.BzhError) as e2:
            dec.grep(broken, NEEDLE)
        assert e1.value.status == e2.value.status == -6 and str(e1.value) == str(e2.value)
    assert dec.grep(bz2.compress(b""), b"a")[0] == b""
    full(dec, inp, NEEDLE)  # the context stays usable


# ---- the indexed call -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sync", [False, True])
def test_grep_index(dec, inp, native, sync):
    pts = inp.pts if sync else None
    dec.search_set_room(1024)  # every block is a window
    try:
        for pat, invert in ((NEEDLE, False), (CARRIED, False), (inp.truth[5000:5003], False), (b"e\n", True)):
            data, got = dec.grep(inp.s, pat, b"\n", invert)
            idata, igot = dec.grep_index(inp.s, inp.ent, pat, pts, b"\n", invert)
            assert idata == data and rows(igot) == rows(got) and data == grep_truth(inp.truth, pat, b"\n", invert)[0]
            st = dec.grep_stats()
            assert st["windows"] >= 5 and st["carry_peak"] > 512
        wrong = inp.ent.copy()
        wrong["end_bit"][2] -= 8  # (the last block of the first stream: the entry stays well formed)
        with pytest.raises(native.BzhError) as err:
            dec.grep_index(inp.s, wrong, NEEDLE, pts)
        assert err.value.status == -6
        assert dec.grep_index(inp.s, inp.ent, NEEDLE, pts, count_only=True)[0] == 5
    finally:
        dec.search_set_room(0)


# ---- one context, every kind of call ---------------------------------------------------------------------------------------------
def test_one_carry_buffer_across_call_kinds(dec, inp, native):
    """A context keeps ONE buffer for what is carried from a window to the next: a search puts its last plen - 1 bytes there, a grep
    its whole open record.  Searches, greps and range searches alternate on one context, every block a window of the indexed walks
    (a room of 1,024) and every batch of two candidates one of the full calls, so the buffer is reused at 2, 11, 16 and more than
    50,000 bytes: the grep for CARRIED carries the long record, far above BZF_FRONT, and the search behind it finds its own short
    carry in the grown buffer.  Every result is what a context that has done nothing else returns."""
    word = inp.truth[5000:5003]
    lo, hi = inp.bounds[0] - 5000, inp.bounds[2] + 5000
    calls = [
        ("search", lambda c: c.search(inp.s, NEEDLE, b"\n")),
        ("grep", lambda c: c.grep(inp.s, word)),
        ("search range", lambda c: c.search_range(inp.s, inp.ent, NEEDLE, lo, hi - lo, inp.pts)),
        ("grep, the hit in the carry", lambda c: c.grep_index(inp.s, inp.ent, CARRIED, inp.pts)),
        ("search behind it", lambda c: c.search(inp.s, CARRIED)),
        ("grep, inverted", lambda c: c.grep_index(inp.s, inp.ent, word, inp.pts, b"\n", True)),
        ("search range, short pattern", lambda c: c.search_range(inp.s, inp.ent, word, lo, hi - lo)),
        ("full grep, the hit in the carry", lambda c: c.grep(inp.s, CARRIED)),
        ("search, short pattern", lambda c: c.search(inp.s, word)),
    ]
    plain = lambda r: tuple(x.tobytes() if isinstance(x, np.ndarray) else x for x in r)
    dec.search_set_room(1024)
    try:
        for name, call in calls:
            got = plain(call(dec))
            if "carry" in name:
                assert dec.grep_stats()["carry_peak"] > 50_000 and dec.grep_stats()["windows"] >= 3, name
            elif "search" in name:
                assert dec.search_stats()["windows"] >= 3, name
            with native.Context(0, 9, 2) as fresh:
                fresh.search_set_room(1024)
                assert got == plain(call(fresh)), name
    finally:
        dec.search_set_room(0)
    hits, nhits = dec.search(inp.s, CARRIED)
    assert nhits == 1 and int(hits[0]["off"]) == inp.long[0] + 100


# ---- Python and the command line -------------------------------------------------------------------------------------------------
def test_python_grep(inp):
    import banzai_amd
    rindex = banzai_amd.build_record_index(inp.s)
    rd = banzai_amd.IndexedReader(inp.s, rindex)
    for pat in (inp.truth[5000:5006], NEEDLE, b"e\n", b"no such bytes anywhere"):
        data, ent = banzai_amd.grep(inp.s, pat)
        old = rd.grep(pat)
        assert [int(r) for r in ent["record"]] == [r for r, _ in old] and data == b"".join(b for _, b in old), pat
        assert banzai_amd.grep_count(inp.s, pat) == len(old)
    # a record is selected or it is not: both greps account for every record and every byte
    pat = inp.truth[5000:5003]
    a, ea = banzai_amd.grep(inp.s, pat)
    b, eb = banzai_amd.grep(inp.s, pat, invert=True)
    assert len(ea) + len(eb) == rindex.nrecords and len(a) + len(b) == len(inp.truth)
    assert sorted(ea["record"].tolist() + eb["record"].tolist()) == list(range(rindex.nrecords))
    whole = bytearray(len(inp.truth))
    for data, ent in ((a, ea), (b, eb)):
        for e in ent:
            whole[int(e["off"]):int(e["off"]) + int(e["len"])] = data[int(e["out_off"]):int(e["out_off"]) + int(e["len"])]
    assert bytes(whole) == inp.truth
    # with an index the indexed front is used
    index = banzai_amd.SyncIndex(banzai_amd.BlockIndex(inp.ent.copy(), len(inp.s)), inp.pts.copy(), 4)
    for ix in (index, index.blocks):
        data, ent = banzai_amd.grep(inp.s, pat, index=ix)
        assert data == a and rows(ent) == rows(ea)
        assert banzai_amd.grep_count(inp.s, pat, invert=True, index=ix) == len(eb)


def test_cli_grep(inp, tmp_path):
    import banzai_amd
    exe = os.path.join(ROOT, "banzai_amd", "bnzhip")
    path, xpath = tmp_path / "t.bz2", tmp_path / "t.bzi"
    path.write_bytes(inp.s)
    xpath.write_bytes(banzai_amd.SyncIndex(banzai_amd.BlockIndex(inp.ent.copy(), len(inp.s)), inp.pts.copy(), 4).to_bytes())
    run = lambda *args: subprocess.run([exe, *args, str(path)], capture_output=True, timeout=120)
    word = inp.truth[5000:5006]
    want, ent, nrec = grep_truth(inp.truth, word)
    p = run("--grep", word.decode())
    assert (p.returncode, p.stdout) == (0, want), p.stderr
    p = run("--grep", word.hex(), "--hex", "--index", str(xpath))
    assert (p.returncode, p.stdout) == (0, want), p.stderr
    p = run("--grep", word.decode(), "--count")
    assert (p.returncode, p.stdout) == (0, b"%d\n" % len(ent)), p.stderr
    inv, ient, _ = grep_truth(inp.truth, word, invert=True)
    p = run("--grep", word.decode(), "--invert", "--count", "--index", str(xpath))
    assert (p.returncode, p.stdout) == (0, b"%d\n" % len(ient)) and len(ent) + len(ient) == nrec, p.stderr
    p = run("--grep", word.decode(), "--invert")
    assert (p.returncode, p.stdout) == (0, inv), p.stderr
    p = run("--grep", NEEDLE.decode(), "--line-number")
    nwant, nent, _ = grep_truth(inp.truth, NEEDLE)
    numbered = b"".join(b"%d:" % (r + 1) + nwant[o:o + n] for r, _, n, o in nent)
    assert (p.returncode, p.stdout) == (0, numbered) and len(nent) == 5, p.stderr
    p = run("--grep", "no such bytes")
    assert (p.returncode, p.stdout) == (0, b""), p.stderr
    p = run("--grep", "a", "--search", "b")
    assert p.returncode != 0 and path.exists()
