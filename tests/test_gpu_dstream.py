"""GPU: the streaming decode (bzh_dstream_*, banzai_amd.StreamDecompressor / decode_stream, bnzhip -d --stream) held to the one-shot
decode of the same bytes: for every chunking and every sequence of cap values the output, consumed, the status and -- for an input
with one defect -- the text of bzh_last_error are bzh_decode's.  Inputs are level-1 streams whose blocks have few symbols (one
block's entropy stage is one serial wavefront)."""
import bz2
import io
import os
import random
import subprocess

import numpy as np
import pytest

import banzai_amd
from tests import cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "banzai_amd", "bnzhip")
OK, E_ARG, E_STATE, E_DATA = 0, -1, -5, -6


def words(n, seed, vocab=40):
    """n bytes of words from a small seeded vocabulary: few symbols, no period"""
    rng = random.Random(seed)
    v = ["".join(rng.choices("etaoinshrdlu", k=rng.randrange(2, 9))) for _ in range(vocab)]
    return " ".join(rng.choices(v, k=n // 3)).encode()[:n]


def stream(ctx, data, feeds, caps, room=None, between=None):
    """`data` through a fresh stream on `ctx` in feeds of the given sizes (an int: all that size; the last one with eof), every
    call with the next of `caps` bytes of room -> (status, bytes handed out, done).  Every call is held to the contract: no more
    used or written than offered, and never nothing done with input or output pending.  between(k): called after feed k."""
    if room:
        ctx.dstream_set_room(*room)
    try:
        ctx.dstream_begin()
    finally:
        if room:
            ctx.dstream_set_room(0, 0)
    if isinstance(feeds, int):
        feeds = [feeds] * (len(data) // feeds) + [len(data) % feeds]
    assert sum(feeds) == len(data)
    bufs = {c: np.empty(c, dtype=np.uint8) for c in set(caps)}
    out, at, calls = [], 0, 0
    for k, size in enumerate(feeds):
        chunk, off, eof = data[at:at + size], 0, k == len(feeds) - 1
        at += size
        while True:
            buf = bufs[caps[calls % len(caps)]]
            calls += 1
            assert calls < 200000, "the feed loop does not end"
            st, used, got, done = ctx.dstream_feed_raw(chunk[off:], eof, buf)
            assert used <= len(chunk) - off and got <= buf.size
            out.append(buf[:got].tobytes())
            if st != OK:
                return st, b"".join(out), False
            assert used or got or done or off == len(chunk), "a feed with input that did nothing"
            off += used
            if done:
                return OK, b"".join(out), True
            if off == len(chunk) and got < buf.size and not eof:
                break
        if between:
            between(k)
    raise AssertionError("the eof feed returned without done")


@pytest.fixture(scope="module")
def three(oracle):
    """three streams back to back -- libbz2's at level 1, the oracle's, an empty one -- and 3 foreign bytes: a few hundred bytes"""
    a, b = words(700, 3), words(500, 4, vocab=12)
    s = bz2.compress(a, 1) + bytes(oracle.encode(b, 1)) + bz2.compress(b"", 1)
    assert len(s) < 1000
    return s + b"\x01\x02\x03", a + b, len(s)


def test_every_split_and_byte_by_byte(ctx1, ctx9, three):
    """every two-chunk split point and byte-at-a-time feeding: output and consumed are bzh_decode's and bz2.decompress's"""
    s, raw, used = three
    assert bz2.decompress(s[:used]) == raw and ctx1.decode(s, with_consumed=True) == (raw, used)
    for k in range(len(s) + 1):
        assert stream(ctx1, s, [k, len(s) - k], [1 << 16]) == (OK, raw, True), k
        assert ctx1.dstream_consumed() == used, k
    for ctx in (ctx1, ctx9):
        assert stream(ctx, s, 1, [1 << 16]) == (OK, raw, True)
        assert ctx.dstream_consumed() == used
        st = ctx.dstream_stats()
        assert (st["streams"], st["in_bytes"], st["out_bytes"]) == (3, used + 3, len(raw)) and st["blocks"] == 2
    # after done: feeds succeed, use everything and change nothing
    buf = np.empty(16, dtype=np.uint8)
    assert ctx1.dstream_feed_raw(b"more", False, buf) == (OK, 4, 0, True)
    ctx1.dstream_end()
    assert ctx1.dstream_feed_raw(b"more", False, buf)[0] == E_STATE
    ctx1.dstream_end()  # (always allowed)


def test_argument_and_sequence_errors(native, ctx1):
    lib = native.lib()
    import ctypes
    used, got, done = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_int(0)
    buf = (ctypes.c_uint8 * 16)()
    fresh = native.Context(0, 1, 8)
    try:
        assert lib.bzh_dstream_feed(fresh.handle, buf, 4, 0, ctypes.byref(used), buf, 16, ctypes.byref(got), ctypes.byref(done)) == E_STATE
        assert lib.bzh_dstream_consumed(fresh.handle) == 0
        assert fresh.dstream_stats()["passes"] == 0
    finally:
        fresh.close()
    ctx1.dstream_begin()
    h = ctx1.handle
    assert lib.bzh_dstream_feed(h, None, 4, 0, ctypes.byref(used), buf, 16, ctypes.byref(got), ctypes.byref(done)) == E_ARG
    assert lib.bzh_dstream_feed(h, buf, 4, 0, ctypes.byref(used), None, 16, ctypes.byref(got), ctypes.byref(done)) == E_ARG
    assert lib.bzh_dstream_feed(h, buf, 4, 0, None, buf, 16, ctypes.byref(got), ctypes.byref(done)) == E_ARG
    assert lib.bzh_dstream_feed(h, buf, 4, 0, ctypes.byref(used), buf, 16, None, ctypes.byref(done)) == E_ARG
    assert lib.bzh_dstream_feed(h, buf, 4, 0, ctypes.byref(used), buf, 16, ctypes.byref(got), None) == E_ARG
    assert lib.bzh_dstream_get_stats(h, None) == E_ARG
    assert lib.bzh_dstream_set_room(h, 1023, 0) == E_ARG and lib.bzh_dstream_set_room(h, 0, 512) == E_ARG
    assert lib.bzh_dstream_set_room(h, 1024, 1024) == OK and lib.bzh_dstream_set_room(h, 0, 0) == OK
    ctx1.dstream_end()


@pytest.fixture(scope="module")
def forty():
    """41 level-1 blocks of the periodic text (165 compressed bytes each), one block of three random symbols -- 20 kB compressed:
    the one item here that no window of 4096 bytes holds, so the one that makes the window grow --, and one block of a single
    byte value whose 5 MB are far beyond the staging target"""
    raw = cases.gen(4_000_000, "text", 1) + cases.gen(95_000, "lowalpha", 2) + cases.gen(5_000_000, "same", 3)
    s = bz2.compress(raw[:4_000_000], 1) + bz2.compress(raw[4_000_000:4_095_000], 1) + bz2.compress(raw[4_095_000:], 1)
    return s, raw


def test_small_rooms_force_every_path(ctx1, forty):
    """a window of 4096 and a staging buffer of 65536 bytes, feeds of 1000 bytes, cap cycling through 1, 4093 and 1 MiB"""
    s, raw = forty
    ent, total, used = ctx1.decode_index(s)
    assert total == len(raw) and len(ent) >= 42
    st, out, done = stream(ctx1, s, 1000, [1, 4093, 1 << 20], room=(4096, 65536))
    assert (st, done) == (OK, True) and out == raw
    assert ctx1.dstream_consumed() == used == len(s)
    d = ctx1.dstream_stats()
    print(d)
    assert d["passes"] > 1 and d["tail_moves"] > 0 and d["window_grows"] > 0 and d["staging_grows"] > 0 and d["blocks_redone"] > 0
    assert d["blocks"] == len(ent) and d["streams"] == 3 and d["in_bytes"] == len(s) and d["out_bytes"] == len(raw)
    largest_in = max((int(e["end_bit"]) - int(e["bit_pos"]) + 7) // 8 + 1 for e in ent)  # (a block begins and ends inside a byte)
    largest_out = max(int(e["out_len"]) for e in ent)
    assert largest_in > 4096 and largest_out > 65536
    assert d["window_peak"] <= max(4096, largest_in) + 1000
    assert d["staging_peak"] <= max(65536, largest_out) + 1000


@pytest.fixture(scope="module")
def good():
    """a level-1 stream of 4 blocks and one of 1 block, back to back"""
    raw = words(350_000, 7) + words(40_000, 8, vocab=15)
    return bz2.compress(raw[:350_000], 1) + bz2.compress(raw[350_000:], 1), raw


def flip(s, bit):
    b = bytearray(s)
    b[bit // 8] ^= 0x80 >> (bit % 8)
    return bytes(b)


def defects(ctx, s):
    ent, _, used = ctx.decode_index(s)
    assert len(ent) == 5 and used == len(s)
    first_end = int(ent[3]["end_bit"])  # the first stream's footer
    rng = random.Random(17)
    yield "a flipped bit in a block payload", flip(s, (int(ent[1]["bit_pos"]) + int(ent[1]["end_bit"])) // 2)
    yield "a damaged block magic", flip(s, int(ent[2]["bit_pos"]) + 13)
    yield "a wrong block CRC", flip(s, int(ent[2]["bit_pos"]) + 48 + 5)
    yield "a wrong stream CRC", flip(s, first_end + 48 + 9)
    for cut in sorted(rng.randrange(5, len(s)) for _ in range(5)):
        yield f"cut at byte {cut}", s[:cut]


@pytest.mark.parametrize("chunking", ["one piece", "feeds of 4999 bytes through small rooms", "two chunks"])
def test_defects_are_named_as_the_one_shot_decode_names_them(ctx1, good, chunking):
    s, raw = good
    items = list(defects(ctx1, s)) + [("a level-9 stream on a level-1 context", s + bz2.compress(b"nine", 9))]
    assert ctx1.decode(s) == raw
    rng = random.Random(5)
    for what, bad in items:
        st1, _, _, _ = ctx1.decode_raw(bad, len(raw) + 6_000_000)  # (room for a damaged block that expands 51-fold)
        want = ctx1.last_error()
        assert st1 in (E_DATA, E_ARG) or (st1 == OK and what.startswith("cut")), what  # (a cut between two streams leaves a good input)
        if chunking == "one piece":
            got = stream(ctx1, bad, [len(bad)], [1 << 20])
        elif chunking == "two chunks":
            k = rng.randrange(len(bad) + 1)
            got = stream(ctx1, bad, [k, len(bad) - k], [65536])
        else:
            got = stream(ctx1, bad, 4999, [1 << 20, 3], room=(4096, 70000))
        text = ctx1.last_error()
        print(what, "|", chunking, "|", st1, want, "|", got[0], text, "|", len(got[1]))
        if st1 == OK:
            assert got == (OK, ctx1.decode(bad), True), what
            continue
        assert got[0] == st1 and text == want, what
        assert raw.startswith(got[1]), what
        buf = np.empty(16, dtype=np.uint8)
        assert ctx1.dstream_feed_raw(b"", True, buf)[0] == E_STATE, what
    assert stream(ctx1, s, 5000, [1 << 20]) == (OK, raw, True)


def test_other_calls_between_two_feeds(ctx1, good, three):
    """between two feeds an encode and a decode on the same context do not disturb the stream (nor it them)"""
    s, raw = good
    small, small_raw, _ = three
    seen = []

    def between(k):
        if k % 3 == 0:
            enc = ctx1.encode(small_raw)
            seen.append(bz2.decompress(bytes(enc)) == small_raw and ctx1.decode(small) == small_raw)

    assert stream(ctx1, s, 7001, [1 << 20, 100], room=(16384, 120000), between=between) == (OK, raw, True)
    assert len(seen) >= 3 and all(seen)


def test_python_and_cli(good, forty, tmp_path):
    s, raw = good
    d = banzai_amd.StreamDecompressor(window=8192, staging=200000)
    parts = []
    for k in range(0, len(s), 3000):
        parts.append(d.decompress(s[k:k + 3000], max_length=50000))
        assert len(parts[-1]) <= 50000
        while not d.needs_input and not d.done:
            parts.append(d.decompress(b"", max_length=50000))
            assert len(parts[-1]) <= 50000
    while not d.done:
        parts.append(d.finish(max_length=77777))
    assert b"".join(parts) == raw and d.done and d.consumed == len(s) and d.stats()["passes"] > 1
    assert d.decompress(b"ignored") == b""
    d.close()
    assert d.consumed == len(s)
    reader, writer = io.BytesIO(s + b"tail"), io.BytesIO()
    assert banzai_amd.decode_stream(reader, writer, chunk=10000) == len(raw) and writer.getvalue() == raw
    bad = flip(s, len(s) * 8 - 100)  # the last stream's footer region: everything in front of it is written first
    writer = io.BytesIO()
    with pytest.raises(banzai_amd.BzhError) as e:
        banzai_amd.decode_stream(io.BytesIO(bad), writer, chunk=10000)
    assert e.value.status == E_DATA and raw.startswith(writer.getvalue())
    # the command line: a pipe, a file, and a damaged file
    r = subprocess.run([BIN, "-d", "--stream", "-c", "-"], input=s, capture_output=True)
    assert r.returncode == 0 and r.stdout == raw, r.stderr
    z = tmp_path / "good.bz2"
    z.write_bytes(s)
    r = subprocess.run([BIN, "-d", "--stream", "-k", str(z)], capture_output=True)
    assert r.returncode == 0 and (tmp_path / "good").read_bytes() == raw and z.exists(), r.stderr
    (tmp_path / "good").unlink()
    r = subprocess.run([BIN, "-d", "--stream", str(z)], capture_output=True)
    assert r.returncode == 0 and (tmp_path / "good").read_bytes() == raw and not z.exists(), r.stderr
    big, big_raw = forty
    cut = big[:len(big) - 20]  # the 5 MB block is cut: the 4 MB in front of it have been decoded by then
    z = tmp_path / "bad.bz2"
    z.write_bytes(cut)
    one = subprocess.run([BIN, "-d", "-k", str(z)], capture_output=True)
    r = subprocess.run([BIN, "-d", "--stream", "-k", str(z)], capture_output=True)
    assert one.returncode == r.returncode == 3 and not (tmp_path / "bad").exists() and z.exists(), r.stderr
    assert r.stderr.strip().splitlines()[-1] == one.stderr.strip().splitlines()[-1]
    r = subprocess.run([BIN, "-d", "--stream", "-c", str(z)], capture_output=True)
    assert r.returncode == 3 and big_raw.startswith(r.stdout)
    assert subprocess.run([BIN, "--stream", str(z)], capture_output=True).returncode == 1
    assert subprocess.run([BIN, "--stream", "--recover", str(z)], capture_output=True).returncode == 1
