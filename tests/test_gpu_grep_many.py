"""GPU: grep over many texts in one device buffer with walls between them (bzh_grep_many_raw_device, bzh_grep_many_device,
bzh_grep_many, their patset twins, banzai_amd.grep_many / grep_many_count, bnzhip --grep with several inputs).  THE RULE under test:
for every input the call returns what bzh_grep returns for that input alone.  The truth is always Python on that one text -- the
raw segment, or bz2.decompress(item) -- cut with split(delim) and searched with bytes.find, or for expressions with `re` under
re.MULTILINE by the rule of tests/regex_look_truth.py; never bzh_grep's own output alone."""
import bisect
import bz2
import os
import random
import subprocess

import numpy as np
import pytest

from tests import regex_look_truth as look
from tests.test_gpu_grep import find_all, grep_truth, on_device, room_on_device, rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 4096
SEGLENS = (0, 1, 15, 16, 17, 4095, 4096, 4097, 8193)
NEEDLE = b"error"
VOCAB = (b"error", b"errors", b"terror", b"err", b"warn:", b"ok", b"x", b"Disk", b"fine", b"a_b", b"42")


@pytest.fixture(scope="module")
def dec(native):
    c = native.Context(0, 9, 2)
    yield c
    c.close()


def words(n, seed, newline=0.12):
    """n bytes of the vocabulary, separated by a blank or, now and then, a newline"""
    rng = random.Random(seed)
    out = bytearray()
    while len(out) < n:
        out += rng.choice(VOCAB) + (b"\n" if rng.random() < newline else b" ")
    return bytes(out[:n])


# ---- the truth: one text at a time ------------------------------------------------------------------------------------------------
def hits_bytes(pat):
    return lambda t: set(find_all(t, pat))


def hits_set(pats):
    return lambda t: {s for p in pats for s in find_all(t, p)}


def hits_regex(exprs):
    return lambda t: {h[0] for h in look.hits(exprs, t)}


def truth_one(t, starts, invert=False, delim=b"\n"):
    """-> (bytes, [(record, off, len, out_off)], nrecords) of the text t whose hit starts are `starts`"""
    cut = t.split(delim)
    recs = [p + delim for p in cut[:-1]] + ([cut[-1]] if cut[-1] else [])
    offs = [0]
    for r in recs:
        offs.append(offs[-1] + len(r))
    hit = {bisect.bisect_right(offs, s) - 1 for s in starts}
    out, ent = bytearray(), []
    for k, r in enumerate(recs):
        if (k in hit) != invert:
            ent.append((k, offs[k], len(r), len(out)))
            out += r
    return bytes(out), ent, len(recs)


def truth_many(texts, hits, invert=False):
    """-> (the call's bytes, the call's entries, the items) of the texts, every one judged alone"""
    out, ent, items = bytearray(), [], []
    for t in texts:
        b, e, nrec = truth_one(t, hits(t), invert)
        ent += [(r, o, n, at + len(out)) for r, o, n, at in e]
        out += b
        items.append((len(t), nrec, len(e), len(b), 0))
    return bytes(out), ent, items


def item_rows(items):
    return [tuple(int(it[f]) for f in ("decoded", "records", "selected", "out_bytes", "status")) for it in items]


def raw_many(dec, buf, offs, lens, pattern, hits, invert=False):
    """bzh_grep_many_raw_device: the counting call, then the exact rooms filled with 0xA5 -- bytes, entries, items against the truth,
    nothing behind the need touched"""
    texts = [buf[o:o + n] for o, n in zip(offs, lens)]
    want, ent, items = truth_many(texts, hits, invert)
    t = on_device(buf)
    assert t.data_ptr() % 16 == 0
    st, nrecs, total, _, got_items = dec.grep_many_raw_device(t.data_ptr(), len(buf), offs, lens, pattern, 0, 0, 0, invert=invert)
    assert (st, nrecs, total) == (0, len(ent), len(want)) and item_rows(got_items) == items, (offs[:4], lens[:4], invert)
    out = room_on_device(len(want))
    st, nrecs, total, got, got_items = dec.grep_many_raw_device(t.data_ptr(), len(buf), offs, lens, pattern, out.data_ptr(), len(want), len(ent),
                                                                invert=invert)
    assert (st, nrecs, total) == (0, len(ent), len(want)) and item_rows(got_items) == items, (offs[:4], lens[:4], invert)
    host = out.cpu().numpy().tobytes()
    assert host[:len(want)] == want and set(host[len(want):]) <= {0xA5}, (offs[:4], lens[:4], invert)
    assert rows(got) == ent, (offs[:4], lens[:4], invert)
    return want, ent, items


def shapes():
    """[(name, buffer, offs, lens)]: the segment shapes of the issue"""
    out = []
    rng = random.Random(11)
    # every length, twice, in a seeded order; the gaps put a segment start on every residue modulo 16
    order = [n for n in SEGLENS if n] * 2
    rng.shuffle(order)
    order[5:5] = [0]
    order.append(0)
    offs, lens, at = [], [], 0
    for n in order:
        at += (len([x for x in lens if x]) % 16 - at) % 16  # (a gap of 0 .. 15 bytes: the j-th non-empty segment starts at residue j modulo 16)
        offs.append(at), lens.append(n)
        at += n
    assert {o % 16 for o, n in zip(offs, lens) if n} == set(range(16))
    buf = bytearray(words(at + 8, 3))
    for o, n in zip(offs, lens):  # the needle at both ends of a segment, and across the wall behind it
        if n >= len(NEEDLE):
            buf[o:o + 5] = NEEDLE
            buf[o + n - 5:o + n] = NEEDLE
        elif n and o >= 2:
            buf[o + n - 2:o + n + 3] = NEEDLE
    assert len(buf) == at + 8
    out.append(("lengths and residues", bytes(buf[:at]), offs, lens))
    # a segment ends on a tile's last byte, the next starts on the next tile's first
    buf = bytearray(words(TILE + 900, 4))
    buf[TILE - 3:TILE + 2] = NEEDLE
    out.append(("a wall on a tile edge", bytes(buf), [100, TILE], [TILE - 100, 900]))
    # 40 segments of 100 bytes in one tile
    out.append(("40 segments in one tile", words(4000, 5, 0.2), [100 * k for k in range(40)], [100] * 40))
    # a gap between two segments, filled with the needle: its bytes are never selected
    buf = bytearray(words(2000, 6))
    buf[900:1100] = (NEEDLE + b"\n") * 33 + b"er"
    out.append(("a gap filled with the needle", bytes(buf), [7, 1100], [893, 900]))
    # a segment of delimiters only; a last byte that is and is not the delimiter
    buf = bytearray(words(900, 7))
    buf[300:600] = b"\n" * 300
    buf[299:300], buf[899:900] = b"\n", b"k"
    out.append(("delimiters only, tail open", bytes(buf), [0, 300, 600], [300, 300, 300]))
    buf[299:300], buf[899:900] = b"k", b"\n"
    out.append(("delimiters only, tail closed", bytes(buf), [0, 300, 600], [300, 300, 300]))
    # a segment without a delimiter over three tiles, its only hit in the first, the middle and the last tile
    for name, where in (("first", 705), ("middle", TILE + 2000), ("last", 700 + 2 * TILE + 900 - 5)):
        buf = bytearray(b". " * ((700 + 2 * TILE + 900 + 300) // 2))
        buf[699:700] = b"\n"
        buf[where:where + 5] = NEEDLE
        out.append((f"three tiles, the hit in the {name}", bytes(buf), [0, 700, 700 + 2 * TILE + 900], [700, 2 * TILE + 900, 300]))
    # the needle cut at every point across a wall
    for cut in range(1, len(NEEDLE)):
        buf = bytearray(b"xy z\n" * 300)
        buf[700 - cut:700 - cut + 5] = NEEDLE
        out.append((f"the needle cut at {cut}", bytes(buf), [200, 700], [500, 800]))
    return out


SHAPES = shapes()


# ---- 1. the raw seam ---------------------------------------------------------------------------------------------------------------
def test_raw_single_pattern(dec):
    for name, buf, offs, lens in SHAPES:
        for invert in (False, True):
            _, ent, _ = raw_many(dec, buf, offs, lens, NEEDLE, hits_bytes(NEEDLE), invert)
            if name.startswith("the needle cut") and not invert:
                assert ent == [], name
    st = dec.grep_many_stats()
    assert st["inputs"] == 2 and st["segments"] == 2 and st["virtual_tiles"] == 2 and st["inputs_failed"] == 0
    # plen 1, 2, 16, 17 and 256 over the lengths: a pattern longer than a segment finds nothing in it
    name, buf, offs, lens = SHAPES[0]
    big = offs[lens.index(8193)]
    for plen in (1, 2, 16, 17, 256):
        pat = buf[big + 4000:big + 4000 + plen]  # (a piece of the long segment)
        raw_many(dec, buf, offs, lens, pat, hits_bytes(pat))


def test_raw_pattern_set(native, dec):
    pats = [b"error", b"warn:", b"Disk ok"]
    with native.PatternSet(dec, pats) as ps:
        for name, buf, offs, lens in SHAPES:
            raw_many(dec, buf, offs, lens, ps, hits_set(pats))
        raw_many(dec, *SHAPES[0][1:], ps, hits_set(pats), invert=True)


@pytest.mark.parametrize("no_lds", [False, True])
def test_raw_regex(native, dec, no_lds):
    exprs = [rb"\berr[a-z]*\b", rb"^warn", rb"ok$"]
    flags = native.REGEX_NO_LDS if no_lds else 0
    with native.PatternSet(dec, exprs, flags=flags, regex=True, syntax=native.REGEX_ASSERT) as rx:
        assert rx.info["in_lds"] == (0 if no_lds else 1) and rx.info["look_ahead"] == 1
        for name, buf, offs, lens in SHAPES:
            raw_many(dec, buf, offs, lens, rx, hits_regex(exprs))
    plain = [rb"err[a-z]+s", rb"[0-9]+ "]
    with native.PatternSet(dec, plain, flags=flags, regex=True) as rx:
        raw_many(dec, *SHAPES[0][1:], rx, hits_regex(plain))
        raw_many(dec, *SHAPES[2][1:], rx, hits_regex(plain), invert=True)


# ---- 2. walls ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("no_lds", [False, True])
def test_walls(native, dec, no_lds):
    a, b = b"one line\nthe last error", b"s and then\na line\n"
    buf = b"\n\n\n" + a + b + b"tail"
    offs, lens = [3, 3 + len(a)], [len(a), len(b)]
    flags = native.REGEX_NO_LDS if no_lds else 0

    def selected(exprs):
        with native.PatternSet(dec, exprs, flags=flags, regex=True, syntax=native.REGEX_ASSERT) as rx:
            _, _, items = raw_many(dec, buf, offs, lens, rx, hits_regex(exprs))
        return [it[2] for it in items]

    for e in (rb"\berror\b", rb"error$", rb"error\Z"):  # the end of segment 0 is the text's end, whatever byte lies behind it
        assert selected([e]) == [1, 0], e
    for e in (rb"^s", rb"\As"):  # the start of segment 1 is the text's start
        assert selected([e]) == [0, 1], e
    assert selected([rb"errors"]) == [0, 0]
    assert raw_many(dec, buf, offs, lens, b"errors", hits_bytes(b"errors"))[1] == []
    # an automaton's walk ends at its segment's end
    c, d = b"x aaa", b"b y\n"
    buf2 = c + d
    with native.PatternSet(dec, [rb"a+b"], flags=flags, regex=True) as rx:
        assert raw_many(dec, buf2, [0, len(c)], [len(c), len(d)], rx, hits_regex([rb"a+b"]))[1] == []
        assert len(raw_many(dec, buf2, [0], [len(buf2)], rx, hits_regex([rb"a+b"]))[1]) == 1  # (one text: the match is there)
    # a set: `ab` ends inside segment 0 and selects it; `abcd` would end in segment 1
    e, f = b"zz ab", b"cd zz\n"
    with native.PatternSet(dec, [b"ab", b"abcd"]) as ps:
        _, _, items = raw_many(dec, e + f, [0, len(e)], [len(e), len(f)], ps, hits_set([b"ab", b"abcd"]))
        assert [it[2] for it in items] == [1, 0]
    with native.PatternSet(dec, [b"abcd"]) as ps:
        assert raw_many(dec, e + f, [0, len(e)], [len(e), len(f)], ps, hits_set([b"abcd"]))[1] == []


# ---- 3. the decode route ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def many_inputs():
    texts = [words(2500 + 37 * k, 100 + k) for k in range(64)]
    texts[9] = b""
    texts[20] = texts[20].rstrip(b"\n") + b" error"  # no final newline
    comp = [bz2.compress(t, 1) for t in texts]
    comp[31] = bz2.compress(texts[31][:1000], 1) + bz2.compress(texts[31][1000:], 1)  # two streams
    return texts, comp


def check_items(items, res, texts, hits, bad=()):
    for k, t in enumerate(texts):
        if k in bad:
            assert item_rows(items[k:k + 1]) == [(0, 0, 0, 0, -6)] and res[k] is None, k
            continue
        want, ent, nrec = truth_one(t, hits(t))
        assert item_rows(items[k:k + 1]) == [(len(t), nrec, len(ent), len(want), 0)], k
        assert res[k][0] == want and rows(res[k][1]) == ent, k


def test_decode_route(native, many_inputs):
    texts, comp = many_inputs
    assert [bz2.decompress(c) for c in comp] == texts
    with native.Context(0, 1, 8) as ctx:
        items, res = ctx.grep_many(comp, NEEDLE)
        check_items(items, res, texts, hits_bytes(NEEDLE))
        st = ctx.grep_many_stats()
        assert st["inputs"] == 64 and st["inputs_failed"] == 0 and st["segments"] == 63 and st["staging_retries"] in (0, 1)
        assert st["virtual_tiles"] >= st["segments"] and st["shared_tiles"] > 0
        counted, none = ctx.grep_many(comp, NEEDLE, count_only=True)
        assert none is None and item_rows(counted) == item_rows(items)
        # the device route: the same inputs in HBM, the exact rooms
        joined = b"".join(comp)
        offs = np.cumsum([0] + [len(c) for c in comp[:-1]]).tolist()
        t = on_device(joined)
        total, nrecs = int(items["out_bytes"].sum()), int(items["selected"].sum())
        out = room_on_device(total)
        got = ctx.grep_many_device(t.data_ptr(), len(joined), offs, [len(c) for c in comp], NEEDLE, out.data_ptr(), total, nrecs)
        assert got[:3] == (0, nrecs, total) and item_rows(got[4]) == item_rows(items)
        host = out.cpu().numpy().tobytes()
        assert host[:total] == b"".join(r[0] for r in res) and set(host[total:]) <= {0xA5}
        # a damaged input fails alone
        hurt = list(comp)
        hurt[5] = comp[5][:len(comp[5]) // 2]
        flipped = bytearray(comp[17])
        flipped[len(flipped) // 2] ^= 0x10
        hurt[17] = bytes(flipped)
        items2, res2 = ctx.grep_many(hurt, NEEDLE)
        check_items(items2, res2, texts, hits_bytes(NEEDLE), bad=(5, 17))
        for k in range(64):
            if k not in (5, 17):
                assert res2[k][0] == res[k][0] and rows(res2[k][1]) == rows(res[k][1]), k
        assert ctx.grep_many_stats()["inputs_failed"] == 2
        # and the context is as usable as before
        items3, res3 = ctx.grep_many(comp[:3], NEEDLE, invert=True)
        for k in range(3):
            want, ent, _ = truth_one(texts[k], hits_bytes(NEEDLE)(texts[k]), invert=True)
            assert res3[k][0] == want and rows(res3[k][1]) == ent


def test_host_out_needs_no_alignment(native, many_inputs):
    """bzh_grep_many writes to a host buffer at any address, as bzh_grep does: only the device variants want 4-byte alignment"""
    import ctypes
    texts, comp = many_inputs
    want = b"".join(truth_one(t, hits_bytes(NEEDLE)(t))[0] for t in texts[:4])
    arrs = [np.frombuffer(c, dtype=np.uint8) for c in comp[:4]]
    ins = (native.u8p * 4)(*[native.ptr(a) for a in arrs])
    lens = np.array([a.size for a in arrs], dtype=np.uint64)
    pat = np.frombuffer(NEEDLE, dtype=np.uint8)
    buf = np.full(len(want) + 8, 0xA5, dtype=np.uint8)
    off = (1 - buf.ctypes.data) % 4  # the output begins at an address that is 1 modulo 4
    items = np.zeros(4, dtype=native.GREP_MANY_ITEM_DTYPE)
    got, total = ctypes.c_size_t(0), ctypes.c_uint64(0)
    with native.Context(0, 1, 8) as ctx:
        st = native.lib().bzh_grep_many(ctx.handle, ins, native.ptr(lens, native.szp), 4, native.ptr(pat), len(NEEDLE), 0, 10,
                                        ctypes.c_void_p(buf.ctypes.data + off), len(want), None, 0, items.ctypes.data_as(native.grepmanyp),
                                        ctypes.byref(got), ctypes.byref(total))
        assert st == 0, ctx.last_error()
    assert total.value == len(want) and buf[off:off + len(want)].tobytes() == want
    assert set(buf[:off].tolist()) | set(buf[off + len(want):].tolist()) <= {0xA5}


def test_staging_retry(native):
    """Inputs that decode to more than the first staging room (six times the compressed bytes and 1 MiB): the staging is sized
    once more from the walk's total and the decode runs again -- never BZH_E_CAP for the call's own staging.  Then the last
    input truncated inside its third block, on a context with batches of 2: its first two blocks were placed before it failed,
    so the walk's total lies beyond the last offset and length; it fails alone."""
    period = b"error: disk full\n" + b"all is fine here\n" * 3
    texts = [period * (2_200_000 // len(period)) + b"tail " + NEEDLE, words(3000, 77), period * (2_100_000 // len(period))]
    comp = [bz2.compress(t, 9) for t in texts]
    assert sum(map(len, texts)) > 6 * sum(map(len, comp)) + (1 << 20)
    with native.Context(0, 9, 2) as ctx:
        items, res = ctx.grep_many(comp, NEEDLE)
        assert ctx.grep_many_stats()["staging_retries"] == 1
        check_items(items, res, texts, hits_bytes(NEEDLE))
        hurt = comp[:2] + [comp[2][:-30]]
        assert len(bz2.BZ2Decompressor().decompress(hurt[2])) == 1_799_963  # (two whole blocks decode, the third is cut)
        items2, res2 = ctx.grep_many(hurt, NEEDLE)
        st = ctx.grep_many_stats()
        assert st["staging_retries"] == 1 and st["inputs_failed"] == 1
        check_items(items2, res2, texts, hits_bytes(NEEDLE), bad=(2,))
        for k in range(2):
            assert res2[k][0] == res[k][0] and rows(res2[k][1]) == rows(res[k][1]), k
        counted, _ = ctx.grep_many(hurt, NEEDLE, count_only=True)
        assert item_rows(counted) == item_rows(items2)


# ---- 4. rooms ---------------------------------------------------------------------------------------------------------------------
def test_rooms(dec):
    name, buf, offs, lens = SHAPES[0]
    want, ent, items = raw_many(dec, buf, offs, lens, NEEDLE, hits_bytes(NEEDLE))
    assert len(ent) > 2
    t = on_device(buf)
    for cap, room in ((len(want) - 1, len(ent)), (len(want), len(ent) - 1)):
        out = room_on_device(len(want))
        st, nrecs, total, got, got_items = dec.grep_many_raw_device(t.data_ptr(), len(buf), offs, lens, NEEDLE, out.data_ptr(), cap, room)
        assert (st, nrecs, total) == (-4, len(ent), len(want)) and item_rows(got_items) == items
        assert set(out.cpu().numpy().tobytes()) <= {0xA5}  # (nothing is gathered)
    # bytes alone, entries alone
    out = room_on_device(len(want))
    st, nrecs, total, got, _ = dec.grep_many_raw_device(t.data_ptr(), len(buf), offs, lens, NEEDLE, out.data_ptr(), len(want), 0)
    assert (st, nrecs, total) == (0, len(ent), len(want)) and out.cpu().numpy().tobytes()[:len(want)] == want
    st, nrecs, total, got, _ = dec.grep_many_raw_device(t.data_ptr(), len(buf), offs, lens, NEEDLE, 0, 0, len(ent))
    assert (st, nrecs, total) == (0, len(ent), len(want)) and rows(got) == ent


# ---- 5. refusals and degenerate calls ------------------------------------------------------------------------------------------------
def test_refusals(dec):
    buf = words(600, 8)
    t = on_device(buf)
    call = lambda offs, lens: dec.grep_many_raw_device(t.data_ptr(), len(buf), offs, lens, NEEDLE, 0, 0, 0)
    dec.grep_set_context(0, 1)
    try:
        assert call([0], [600])[0] == -1 and "context" in dec.last_error()
    finally:
        dec.grep_set_context(0, 0)
    assert call([], [])[:3] == (0, 0, 0)
    assert call([0, 5], [6, 2])[0] == -1 and "segment 1" in dec.last_error() and "overlap" in dec.last_error()
    assert call([8, 2], [2, 2])[0] == -1 and "segment 1" in dec.last_error()
    assert call([0, 599], [2, 2])[0] == -1 and "segment 1" in dec.last_error() and "past the end" in dec.last_error()
    assert dec.grep_many_raw_device(t.data_ptr() + 4, 100, [0], [100], NEEDLE, 0, 0, 0)[0] == -1 and "16-byte" in dec.last_error()
    # more virtual tiles than one launch takes: refused from the segment table alone, before a byte of the buffer is read
    assert dec.grep_many_raw_device(t.data_ptr(), 1 << 45, [0], [1 << 44], NEEDLE, 0, 0, 0)[0] == -1 and "virtual tiles" in dec.last_error()
    st, nrecs, _, _, items = call([0, 300], [300, 300])  # the context stays usable
    assert st == 0 and nrecs == sum(len(truth_one(x, hits_bytes(NEEDLE)(x))[1]) for x in (buf[:300], buf[300:]))


# ---- 6. Python ---------------------------------------------------------------------------------------------------------------------
def test_python(native, many_inputs):
    import banzai_amd
    texts, comp = many_inputs
    some = comp[:12] + [comp[20], comp[31]]
    for pattern in (NEEDLE, banzai_amd.PatternSet([b"error", b"warn:"]), banzai_amd.Regex([rb"\berror\b", rb"^Disk"]), banzai_amd.Regex(rb"ok$", _no_lds=True)):
        got = banzai_amd.grep_many(some, pattern)
        one = [banzai_amd.grep(x, pattern) for x in some]
        assert [(g[0], rows(g[1])) for g in got] == [(o[0], rows(o[1])) for o in one]
        assert banzai_amd.grep_many_count(some, pattern) == [banzai_amd.grep_count(x, pattern) for x in some]
        assert banzai_amd.grep_many_count(some, pattern, invert=True) == [banzai_amd.grep_count(x, pattern, invert=True) for x in some]
    want = [truth_one(t, hits_bytes(NEEDLE)(t)) for t in texts[:12]]  # (and against the truth, not bzh_grep's word alone)
    assert [g[0] for g in banzai_amd.grep_many(comp[:12], NEEDLE)] == [w[0] for w in want]
    hurt = [comp[0], comp[1][:40], comp[2]]
    with pytest.raises(native.BzhError) as e:
        banzai_amd.grep_many(hurt, NEEDLE)
    assert e.value.status == -6 and "item 1 of grep_many" in str(e.value)
    got = banzai_amd.grep_many(hurt, NEEDLE, errors="return")
    assert isinstance(got[1], native.BzhError) and got[1].status == -6
    assert got[0][0] == want[0][0] and got[2][0] == want[2][0]
    counts = banzai_amd.grep_many_count(hurt, NEEDLE, errors="return")
    assert counts[0] == len(want[0][1]) and isinstance(counts[1], native.BzhError) and counts[2] == len(want[2][1])
    assert banzai_amd.grep_many([], NEEDLE) == []


# ---- 7. the CLI ---------------------------------------------------------------------------------------------------------------------
def test_cli(native, tmp_path):
    exe = os.path.join(ROOT, "banzai_amd", "bnzhip")
    texts = [words(3000, 41), b"nothing to see\nhere\n", words(5000, 42).rstrip(b"\n") + b" error"]
    names = [str(tmp_path / f"f{k}.bz2") for k in range(3)]
    for n, t in zip(names, texts):
        with open(n, "wb") as f:
            f.write(bz2.compress(t))
    run = lambda *args: subprocess.run([exe, *args], capture_output=True, timeout=120)

    def expect(select, number=False, count=False, prefix=True):
        out = bytearray()
        for n, t in zip(names, texts):
            head = (n.encode() + b":") if prefix else b""
            lines = [(k, ln) for k, ln in enumerate(t.split(b"\n")[:-1] + ([t.split(b"\n")[-1]] if not t.endswith(b"\n") else [])) if select(ln)]
            if count:
                out += head + b"%d\n" % len(lines)
                continue
            for k, ln in lines:
                out += head + (b"%d:" % (k + 1) if number else b"") + ln + b"\n"
        return bytes(out)

    has = lambda ln: NEEDLE in ln
    p = run("--grep", "error", *names)
    assert p.returncode == 0 and p.stdout == expect(has), p.stderr
    p = run("--grep", "error", "--line-number", *names)
    assert p.returncode == 0 and p.stdout == expect(has, number=True)
    p = run("--grep", "error", "--count", *names)
    assert p.returncode == 0 and p.stdout == expect(has, count=True) and names[1].encode() + b":0\n" in p.stdout
    p = run("--grep", "error", "--no-filename", *names)
    assert p.returncode == 0 and p.stdout == expect(has, prefix=False)
    p = run("--grep", "^[A-Z]", "-E", *names)
    assert p.returncode == 0 and p.stdout == expect(lambda ln: ln[:1].isupper() and ln[:1].isalpha())
    p = run("--grep", "error", "--invert", "--count", *names)
    assert p.returncode == 0 and p.stdout == expect(lambda ln: not has(ln), count=True)
    # a fourth, damaged file: the others' output is unchanged, its name is on standard error, the exit status is ERR_OUTPUT
    bad = str(tmp_path / "bad.bz2")
    with open(bad, "wb") as f:
        f.write(bz2.compress(texts[0])[:-20])
    p = run("--grep", "error", names[0], bad, names[1], names[2])
    assert p.returncode == 3 and p.stdout == expect(has) and bad.encode() in p.stderr and names[0].encode() not in p.stderr
    missing = str(tmp_path / "missing.bz2")
    p = run("--grep", "error", *names, missing)
    assert p.returncode == 3 and p.stdout == expect(has) and missing.encode() in p.stderr
    # what several inputs do not go with, and every other mode
    p = run("--grep", "error", "-o", names[0], names[1])
    assert p.returncode == 1 and b"'-o'" in p.stderr and p.stdout == b""
    p = run("--grep", "error", "-A", "1", names[0], names[1])
    assert p.returncode == 1 and b"'-A'" in p.stderr
    p = run("--search", "error", names[0], names[1])
    assert p.returncode == 1 and b"Only one input may be specified" in p.stderr
    p = run("-d", "-c", names[0], names[1])
    assert p.returncode == 1 and b"Only one input may be specified" in p.stderr
    # a single input keeps its output: no name, the last line as it is
    p = run("--grep", "error", names[2])
    assert p.returncode == 0 and p.stdout == grep_truth(texts[2], NEEDLE)[0] and not p.stdout.endswith(b"\n")
