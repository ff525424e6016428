"""GPU: random access into .bz2 -- the verified block index (bzh_decode_index*) and the decode of a byte range from only the
blocks it touches (bzh_decode_range*, banzai_amd.decompress_range, IndexedReader).  The truth is bz2.decompress(stream)[off:off+len]
throughout.  Damaged inputs come last and are a short fixed list: the wide mutation of the shared per-thread logic runs on the
host build (tests/test_index_api.py)."""
import bz2
import functools
import io
import json
import os
import random

import numpy as np
import pytest

from tests import bz2_handbuilt, cases, rle_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BLOCK_MAGIC = 0x314159265359


@pytest.fixture(scope="module")
def dec(native):
    """the decoding context: level 9 (every stream's level fits), batches of 8 blocks"""
    c = native.Context(0, 9, 8)
    yield c
    c.close()


@pytest.fixture(scope="module")
def four(dec):
    """a level-1 stream of 350,000 bytes (4 blocks), its truth and its index -- computed once, never changed"""
    s = bz2.compress(text(350_000, 41, words=40), 1)
    truth = bz2.decompress(s)
    ent, total, used = dec.decode_index(s)
    assert len(ent) == 4 and total == len(truth) and used == len(s)
    ent.setflags(write=False)
    return s, truth, ent


@functools.lru_cache(maxsize=None)
def text(n, seed, words=3000):
    """n bytes of words drawn from a seeded vocabulary: compresses like text and, unlike cases.gen's "text", differs with the
    seed and has no period.  A small vocabulary leaves fewer symbols for the entropy stage -- one serial wavefront a block,
    which is nearly all a range read costs -- so the tests that make hundreds of reads use one."""
    rng = random.Random(seed)
    vocab = ["".join(rng.choices("etaoinshrdlucmfwypvbgkqjxz", k=rng.randrange(2, 11))) for _ in range(words)]
    return " ".join(rng.choices(vocab, k=n // 4)).encode()[:n]


def bits_at(s, bit, n):
    """n <= 64 bits of `s` from bit position `bit`, MSB first"""
    chunk = s[bit // 8:bit // 8 + 10]
    v = int.from_bytes(chunk + bytes(10 - len(chunk)), "big")
    return (v >> (80 - bit % 8 - n)) & ((1 << n) - 1)


def check_index(dec, s, streams_with_blocks=None):
    truth = bz2.decompress(s)
    ent, total, used = dec.decode_index(s)
    st = dec.decode_stats()
    assert total == len(truth) and st["blocks"] == len(ent) and st["out_bytes"] == total
    assert dec.decode(s, with_consumed=True) == (truth, used)
    off = 0
    for k, e in enumerate(ent):
        assert bits_at(s, int(e["bit_pos"]), 48) == BLOCK_MAGIC, k
        assert bits_at(s, int(e["bit_pos"]) + 48, 32) == int(e["crc"]), k
        assert int(e["out_off"]) == off and int(e["out_len"]) > 0, k
        if k and ent[k - 1]["stream"] == e["stream"]:
            assert int(ent[k - 1]["end_bit"]) == int(e["bit_pos"]), k
        elif k:
            assert int(e["stream"]) > int(ent[k - 1]["stream"]) and int(e["bit_pos"]) > int(ent[k - 1]["end_bit"]), k
        lo = int(e["bit_pos"]) // 8
        assert bits_at(s, int(e["end_bit"]), 48) in (BLOCK_MAGIC, 0x177245385090), k  # a block or the footer follows
        piece = truth[off:off + int(e["out_len"])]
        assert dec.decode_range(s, ent, off, int(e["out_len"])) == piece, k
        assert dec.decode_stats()["blocks"] == 1 and dec.decode_stats()["candidates"] == 0
        assert dec.crc32(piece) == int(e["crc"]), k
        assert 1 <= int(e["level"]) <= 9 and lo < len(s)
        off += int(e["out_len"])
    assert off == len(truth)
    if streams_with_blocks is not None:
        assert sorted(set(ent["stream"].tolist())) == streams_with_blocks
    return ent, truth


# ---- 1. the index is right ---------------------------------------------------------------------------------------------
def test_index_of_libbz2_and_own_streams(dec, ctx1, ctx9):
    d = text(350_000, 41)
    ent, _ = check_index(dec, bz2.compress(d, 1))
    assert len(ent) == 4 and set(ent["level"].tolist()) == {1}
    for fixed in (False, True):
        ctx1.set_mode(fixed)
        try:
            s = ctx1.encode(d)
        finally:
            ctx1.set_mode(False)
        assert len(check_index(dec, s)[0]) == 4
    big = text(1_200_000, 42)
    ent, _ = check_index(dec, ctx9.encode(big))
    assert len(ent) == 2 and set(ent["level"].tolist()) == {9}
    assert len(check_index(dec, bz2.compress(big, 9))[0]) == 2
    ent, total, used = dec.decode_index(bz2.compress(b"", 9))  # an empty stream: no entry
    assert len(ent) == 0 and total == 0 and used == 14


def test_index_of_golden_streams(dec):
    v = json.load(open(os.path.join(GOLDEN, "streams.json")))["streams"]
    assert v
    for c in v:
        check_index(dec, bytes.fromhex(c["stream_hex"]))


def test_index_of_concatenated_streams(dec):
    parts = [(text(350_000, 1), 1), (cases.gen(200_000, "shortruns", 2), 9), (b"", 5),
             (cases.gen(450_000, "longruns", 3), 3), (cases.gen(120_000, "random", 4), 1)]
    body = b"".join(bz2.compress(d, lv) for d, lv in parts)
    s = body + b"\x00foreign"[:7]
    ent, truth = check_index(dec, s, streams_with_blocks=[0, 1, 3, 4])  # the empty stream in the middle has no entry
    assert truth == b"".join(d for d, _ in parts)
    assert dec.decode_index(s)[2] == len(body)
    for stream, (_, lv) in enumerate(parts):
        assert all(int(e["level"]) == lv for e in ent if e["stream"] == stream)
    # ranges across the seams of the streams
    for k in range(1, len(ent)):
        b = int(ent[k]["out_off"])
        assert dec.decode_range(s, ent, b - 3, 7) == truth[b - 3:b + 4]
    import banzai_amd
    ix = banzai_amd.build_index(s)
    assert ix.entries.tobytes() == ent.tobytes() and ix.size == len(truth) and ix.consumed == len(body) and len(ix) == len(ent)
    assert banzai_amd.BlockIndex.from_bytes(ix.to_bytes()).entries.tobytes() == ent.tobytes()
    assert banzai_amd.decompress_range(s, ix, 349_990, 30) == truth[349_990:350_020]
    assert banzai_amd.decompress_range(bytearray(s), ix, 0, 10 ** 9) == truth


def test_index_capacity(dec, native, four):
    import ctypes
    s, truth, ent = four
    src = np.frombuffer(s, dtype=np.uint8)
    cnt, used, total = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_uint64(0)
    for room in (0, 3):
        buf = np.zeros(max(room, 1), dtype=native.INDEX_DTYPE)
        st = native.lib().bzh_decode_index(dec.handle, native.ptr(src), len(s), buf.ctypes.data_as(native.idxp) if room else None, room,
                                           ctypes.byref(cnt), ctypes.byref(total), ctypes.byref(used))
        assert st == -4 and cnt.value == 4 and total.value == len(truth)
    assert dec.decode_index(s)[0].tobytes() == ent.tobytes()


# ---- 2. windows at every edge ------------------------------------------------------------------------------------------
def test_windows_at_every_block_edge(dec, native, four):
    s, truth, ent = four
    total = len(truth)
    pairs = []
    for k in range(1, 4):
        b, blen = int(ent[k]["out_off"]), int(ent[k]["out_len"])
        for off in range(b - 2, b + 3):
            pairs += [(off, n) for n in (0, 1, 2, 3, 4, 5, 4095, 4096, 4097, blen, blen + 1)]
    blen = int(ent[0]["out_len"])
    for off in (0, total - 1, total, total + 5):
        pairs += [(off, n) for n in (0, 1, 2, 3, 4, 5, 4095, 4096, 4097, blen, blen + 1, total, total + 9)]
    rng = random.Random(2024)
    pairs += [(rng.randrange(total), rng.randrange(rng.choice([10, 5000, total]))) for _ in range(200)]
    for off, n in pairs:
        got = dec.decode_range(s, ent, off, n)
        assert got == truth[off:off + n], (off, n)
        first, last, _, _ = native.index_span(ent, off, n)
        st = dec.decode_stats()
        assert st["blocks"] == last - first and st["candidates"] == 0 and st["out_bytes"] == len(got), (off, n)


def test_windows_in_level9_blocks(dec, ctx9):
    d = text(1_200_000, 43)
    s = ctx9.encode(d)
    ent, total, _ = dec.decode_index(s)
    assert len(ent) == 2 and total == len(d)
    b = int(ent[1]["out_off"])
    for off, n in ((b - 1, 1), (b - 1, 2), (b, 1), (b - 4097, 8194), (0, 1), (total - 1, 1), (5, b), (b - 7, total), (0, total)):
        assert dec.decode_range(s, ent, off, n) == d[off:off + n], (off, n)


# ---- 3. runs and unstaged tiles ----------------------------------------------------------------------------------------
def test_runs_and_unstaged_tiles(dec):
    """255-byte runs of alternating bytes: every 4,096 bytes behind the inverse BWT expand past the 8 KiB the walk stages, so
    the tile takes the byte-store path; text behind them, so that staged and unstaged tiles meet"""
    runs = 830
    d = b"".join(bytes([97 + k % 2]) * 255 for k in range(runs)) + text(2_500, 44, words=40)
    s = bz2.compress(d, 1)
    ent, total, _ = dec.decode_index(s)
    assert len(ent) == 1 and total == len(d)
    # the output offset where byte 4,096 behind the inverse BWT begins: the runs before it, and how far into its run it lies
    per = rle_model.canon_len(255)
    assert per == 5  # four bytes and a count
    run, inside = divmod(4096, per)
    seam = run * 255 + min(inside, 4)  # bytes 0..3 of a run's five stand for one byte each, the fifth for the other 251
    assert seam == 819 * 255 + 1
    assert per * runs < 8192 and 255 * (per * runs - 4096) // per + 2_500 <= 8192  # tile 0 is unstaged, tile 1 (runs, then text) staged
    seam2 = 255 * runs  # where the text begins, inside the staged tile
    starts = list(range(0, 600)) + list(range(seam - 300, seam + 301)) + list(range(seam2 - 20, seam2 + 21))
    for off in starts:
        for n in (1, 7, 300, 10_000):
            assert dec.decode_range(s, ent, off, n) == d[off:off + n], (off, n)


# ---- 4. edge blocks ----------------------------------------------------------------------------------------------------
def edge_windows(total):
    for off in list(range(0, 5)) + list(range(total - 5, total)):
        for n in (1, 2, 3, 4, 5, 6):
            yield off, n
    yield 0, total
    yield 1, total - 2


def test_edge_blocks(dec):
    full = bz2_handbuilt.stream_of_rle((b"aaaa\xff" + b"bbbb\xfe") * 10000, 1)  # nblock = 100,000: one more than encoders fill
    want = (b"a" * 259 + b"b" * 258) * 10000
    ent, total, _ = dec.decode_index(full)
    assert len(ent) == 1 and total == len(want) == 5_170_000
    for off, n in edge_windows(total):
        assert dec.decode_range(full, ent, off, n) == want[off:off + n], (off, n)
    for off in (258, 259, 260, 516, 517, 518, 2_585_000):
        assert dec.decode_range(full, ent, off, 600) == want[off:off + 600], off
    tail = text(30_000, 45) + b"z" * 100  # the block's data ends in a run with a count byte
    s = bz2.compress(tail, 1)
    ent, total, _ = dec.decode_index(s)
    assert len(ent) == 1 and total == len(tail)
    for off, n in edge_windows(total):
        assert dec.decode_range(s, ent, off, n) == tail[off:off + n], (off, n)
    zero = bz2_handbuilt.stream_of_rle(b"qrszzzz\x00", 1)  # ... and in a count of zero
    ent, total, _ = dec.decode_index(zero)
    assert total == 7
    for off in range(8):
        for n in range(9):
            assert dec.decode_range(zero, ent, off, n) == b"qrszzzz"[off:off + n]


# ---- 5. partial buffer -------------------------------------------------------------------------------------------------
def test_partial_buffer(dec, native, four):
    s, truth, ent = four
    b2, b3 = int(ent[2]["out_off"]), int(ent[3]["out_off"])
    for off, n in ((b2 + 10, 50), (b2 - 1, 2), (b2 - 5, b3 - b2 + 10), (0, 3), (len(truth) - 3, 3), (100, len(truth))):
        first, last, lo, hi = native.index_span(ent, off, n)
        assert 0 <= lo < hi <= len(s)
        whole = dec.decode_range(s, ent, off, n)
        assert whole == truth[off:off + n]
        assert dec.decode_range(s[lo:hi], ent, off, n, in_byte_base=lo) == whole
        assert dec.decode_range(s[lo:], ent, off, n, in_byte_base=lo) == whole
        for short, base in ((s[lo:hi - 1], lo), (s[lo + 1:hi], lo + 1)):
            with pytest.raises(native.BzhError) as e:
                dec.decode_range(short, ent, off, n, in_byte_base=base)
            assert e.value.status == -1 and f"{first}..{last - 1}" in str(e.value)
            assert dec.decode_range(s[lo:hi], ent, off, n, in_byte_base=lo) == whole  # the context goes on


def test_ill_formed_index_and_small_buffer(dec, native, four, ctx9):
    s, truth, ent = four
    for field, k, value in (("bit_pos", 2, int(ent[1]["bit_pos"])), ("end_bit", 1, int(ent[1]["bit_pos"])), ("out_off", 3, 5),
                            ("level", 0, 0), ("level", 2, 10)):
        bad = ent.copy()
        bad[field][k] = value
        with pytest.raises(native.BzhError) as e:
            dec.decode_range(s, bad, 0, 10)  # (the range does not touch the entry: the index is checked as a whole)
        assert e.value.status == -1 and f"entry {k}" in str(e.value), field
    # offsets that do not start at 0 (a slice of an index), with a range in front of, inside and across the first entry
    late = ent[1:].copy()
    for off, n in ((0, 10), (int(late[0]["out_off"]) - 5, 10), (int(late[0]["out_off"]) + 5, 10), (0, len(truth))):
        with pytest.raises(native.BzhError) as e:
            dec.decode_range(s, late, off, n)
        assert e.value.status == -1 and "entry 0" in str(e.value) and "running sum" in str(e.value), (off, n)
    one = ent[:1].copy()
    one["out_off"] = 100
    with pytest.raises(native.BzhError) as e:
        dec.decode_range(s, one, 50, 10)
    assert e.value.status == -1 and "entry 0" in str(e.value)
    assert dec.decode_range(s, ent, 3, 10) == truth[3:13]
    with native.Context(0, 1, 4) as c1:  # an entry above the context's level is the caller's error
        big = ctx9.encode(text(50_000, 46))
        ent9, _, _ = dec.decode_index(big)
        with pytest.raises(native.BzhError) as e:
            c1.decode_range(big, ent9, 0, 10)
        assert e.value.status == -1 and "level" in str(e.value)
        assert c1.decode_range(s, ent, 7, 10) == truth[7:17]
    # cap below the range: BZH_E_ARG, nothing written
    import ctypes
    src = np.frombuffer(s, dtype=np.uint8)
    out = np.full(64, 0xA5, dtype=np.uint8)
    got = ctypes.c_size_t(0)
    e_arr = np.ascontiguousarray(ent)
    st = native.lib().bzh_decode_range(dec.handle, native.ptr(src), len(s), 0, e_arr.ctypes.data_as(native.idxp), 4, 10, 32, native.ptr(out),
                                       31, ctypes.byref(got))
    assert st == -1 and got.value == 0 and (out == 0xA5).all()
    st = native.lib().bzh_decode_range(dec.handle, native.ptr(src), len(s), 0, e_arr.ctypes.data_as(native.idxp), 4, 10, 32, native.ptr(out),
                                       32, ctypes.byref(got))
    assert st == 0 and got.value == 32 and out[:32].tobytes() == truth[10:42] and (out[32:] == 0xA5).all()


# ---- 6. device variant -------------------------------------------------------------------------------------------------
def test_device_variant_writes_nothing_outside(dec, native, four):
    import torch
    s, truth, ent = four
    t_in = torch.frombuffer(bytearray(s), dtype=torch.uint8).cuda()
    b1, l1 = int(ent[1]["out_off"]), int(ent[1]["out_len"])
    windows = [(b1, 1), (b1, 5), (b1, 4097), (b1 + l1 // 2, 1), (b1 + l1 // 2 - 3, 9001), (b1 + l1 - 1, 1), (b1 + l1 - 5, 5),
               (b1 + l1 - 4097, 4097), (b1, l1), (b1 - 1, l1 + 2), (b1 + 1, l1 - 2), (b1 - 3, 6), (0, len(truth)), (3, len(truth) - 6),
               (b1 + 1, 2 * l1)]
    for off, n in windows:
        want = truth[off:off + n]
        for shift in (0, 1, 2, 3):  # every alignment of the output's first byte
            t_out = torch.full((64 + shift + len(want) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            got = dec.decode_range_device(t_in.data_ptr(), len(s), ent, off, n, t_out.data_ptr() + 64 + shift, len(want))
            h = t_out.cpu().numpy()
            assert got == len(want) and h[64 + shift:64 + shift + got].tobytes() == want, (off, n, shift)
            assert (h[:64 + shift] == 0xA5).all() and (h[64 + shift + got:] == 0xA5).all(), (off, n, shift)
    # the span alone, resident, with its base
    first, last, lo, hi = native.index_span(ent, b1 + 10, 100)
    t_span = torch.frombuffer(bytearray(s[lo:hi]), dtype=torch.uint8).cuda()
    t_out = torch.full((228,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert dec.decode_range_device(t_span.data_ptr(), hi - lo, ent, b1 + 10, 100, t_out.data_ptr() + 64, 100, in_byte_base=lo) == 100
    h = t_out.cpu().numpy()
    assert h[64:164].tobytes() == truth[b1 + 10:b1 + 110] and (h[:64] == 0xA5).all() and (h[164:] == 0xA5).all()


# ---- 8. IndexedReader --------------------------------------------------------------------------------------------------
class CountingFile:
    """a seekable binary file that counts the bytes read from it"""

    def __init__(self, data):
        self.f = io.BytesIO(data)
        self.bytes_read = 0

    def seek(self, *a):
        return self.f.seek(*a)

    def tell(self):
        return self.f.tell()

    def read(self, n=-1):
        out = self.f.read(n)
        self.bytes_read += len(out)
        return out


def test_indexed_reader(dec, four):
    import banzai_amd
    s, truth, ent = four
    src = CountingFile(s)
    r = banzai_amd.IndexedReader(src)  # no index given: the source is read once and indexed
    assert src.bytes_read == len(s) and r.index.entries.tobytes() == ent.tobytes() and r.size == len(truth)
    ix = banzai_amd.BlockIndex.from_bytes(r.index.to_bytes())
    src = CountingFile(s)
    r = banzai_amd.IndexedReader(src, ix)
    ref = io.BytesIO(truth)
    assert src.bytes_read == 0 and r.readable() and r.seekable() and r.tell() == 0
    b2 = int(ent[2]["out_off"])
    script = [("read", 10), ("read", 4096), ("seek", b2 - 3, 0), ("read", 6), ("readinto", 5000), ("seek", -100, 2), ("read", 50),
              ("read", 500), ("read", 5), ("seek", 17, 0), ("seek", 1000, 1), ("readinto", 1), ("seek", 150_000, 1), ("seek", -20_000, 1),
              ("read", 120_000),
              ("seek", 0, 2), ("read", 10), ("seek", len(truth) + 50, 0), ("read", 10), ("readinto", 7), ("seek", 5, 0), ("read", 0),
              ("seek", b2, 0), ("read", -1)]
    for step in script:
        if step[0] == "seek":
            assert r.seek(step[1], step[2]) == ref.seek(step[1], step[2]) == r.tell()
            continue
        pos, before = r.tell(), src.bytes_read
        if step[0] == "read":
            got, want = r.read(step[1]), ref.read(step[1])
        else:
            a, b = bytearray(step[1]), bytearray(step[1])
            na, nb = r.readinto(a), ref.readinto(b)
            assert na == nb
            got, want = bytes(a[:na]), bytes(b[:nb])
        assert got == want and r.tell() == ref.tell(), step
        _, _, lo, hi = ix.span(pos, len(want))
        assert src.bytes_read - before == hi - lo, step  # only the span of this read was fetched
    r = banzai_amd.IndexedReader(s, ix)  # bytes as the source
    r.seek(b2 - 1)
    assert r.read(3) == truth[b2 - 1:b2 + 2] and r.read() == truth[b2 + 2:] and r.read(1) == b""
    assert banzai_amd.IndexedReader(memoryview(s)).read() == truth
    buffered = io.BufferedReader(banzai_amd.IndexedReader(s, ix), buffer_size=8192)
    buffered.seek(b2 - 10)
    assert buffered.read(20) == truth[b2 - 10:b2 + 10]


# ---- 7. mismatch is a status, never a fault (after everything valid) ----------------------------------------------------
def test_mismatch_is_a_status(dec, native, four):
    import banzai_amd
    s, truth, ent = four
    total = len(truth)

    def refused(data, entries, off, n, entry, what=None):
        with pytest.raises(native.BzhError) as e:
            dec.decode_range(data, entries, off, n)
        assert e.value.status == -6 and f"index entry {entry} " in str(e.value), str(e.value)
        if what:
            assert what in str(e.value), str(e.value)
        assert dec.decode_range(s, ent, 5, 20) == truth[5:25]  # the context goes on

    # the index of stream A with stream B of the same length
    other = bz2.compress(text(350_000, 99, words=40), 1)
    size = max(len(s), len(other))
    a, b = s + bytes(size - len(s)), other + bytes(size - len(other))
    assert len(a) == len(b) and dec.decode_index(a)[0].tobytes() == ent.tobytes()  # (zero bytes behind a stream are foreign)
    with pytest.raises(native.BzhError) as e:
        dec.decode_range(b, ent, 0, total)
    assert e.value.status == -6
    refused(b, ent, int(ent[2]["out_off"]) + 5, 10, 2)
    # one entry that does not describe its block
    off1 = int(ent[1]["out_off"])
    for field, delta, what in (("bit_pos", 1, None), ("bit_pos", -1, None), ("end_bit", 8, "end_bit"), ("crc", None, "stored CRC"),
                               ("out_len", 1, "size")):
        bad = ent.copy()
        bad[field][1] = int(bad[field][1]) ^ 1 if delta is None else int(bad[field][1]) + delta
        if field == "out_len":  # (the index stays well formed: the offsets behind the entry move along)
            bad["out_off"][2:] += 1
        refused(s, bad, off1 + 100, 10, 1, what)
        refused(s, bad, off1 - 1, 2, 1, what)
        assert dec.decode_range(s, bad, 10, 100) == truth[10:110]  # block 0 is what its entry says
    # one flipped bit in the stored CRC of block 2
    flip = int(ent[2]["bit_pos"]) + 48 + 13
    damaged = bytearray(s)
    damaged[flip // 8] ^= 0x80 >> (flip % 8)
    damaged = bytes(damaged)
    off2, off3 = int(ent[2]["out_off"]), int(ent[3]["out_off"])
    assert dec.decode_range(damaged, ent, 0, off1) == truth[:off1]
    assert dec.decode_range(damaged, ent, off1 + 3, off2 - off1 - 3) == truth[off1 + 3:off2]
    assert dec.decode_range(damaged, ent, off3, total) == truth[off3:]  # damage in a block the range does not touch is not seen
    with pytest.raises(native.BzhError) as e:
        dec.decode_range(damaged, ent, off2 - 1, 2)
    assert e.value.status == -6 and "index entry 2 " in str(e.value) and "stored CRC" in str(e.value)
    # with the damaged CRC in the entry as well, the computed CRC is what differs: the range sees it from the block alone
    trusting = ent.copy()
    trusting["crc"][2] = bits_at(damaged, int(ent[2]["bit_pos"]) + 48, 32)
    for off, n in ((off2 + 10, 10), (off2, off3 - off2), (off2 - 1, 2)):  # clipped, whole and cut at its head
        with pytest.raises(native.BzhError) as e:
            dec.decode_range(damaged, trusting, off, n)
        assert e.value.status == -6 and "index entry 2 " in str(e.value) and "block CRC mismatch" in str(e.value)
    # the index build verifies block CRCs with no output buffer: the same verdict as the full decode's
    with pytest.raises(native.BzhError) as e_full:
        dec.decode(damaged, size_hint=total)  # (room for the output: a sizing call verifies no block CRC)
    with pytest.raises(native.BzhError) as e_index:
        dec.decode_index(damaged)
    with pytest.raises(native.BzhError) as e_py:
        banzai_amd.build_index(damaged)
    for e in (e_full, e_index, e_py):
        assert e.value.status == -6 and "block CRC mismatch" in str(e.value) and "block 2" in str(e.value)
    assert dec.decode_index(s)[0].tobytes() == ent.tobytes()


def test_crc_verdict_order(dec, native, four):
    """Two blocks of one batch whose computed CRCs differ from their entries': a single range reads the verdicts of the whole
    blocks first, then those of the cut ones; decode_ranges reads them in ascending entry order."""
    s, truth, ent = four
    damaged = bytearray(s)
    for k in (0, 1):  # one flipped bit in the stored CRC of blocks 0 and 1 ...
        flip = int(ent[k]["bit_pos"]) + 48 + 13
        damaged[flip // 8] ^= 0x80 >> (flip % 8)
    damaged = bytes(damaged)
    trusting = ent.copy()
    for k in (0, 1):  # ... and the damaged CRCs in the entries as well: the computed CRC is what differs
        trusting["crc"][k] = bits_at(damaged, int(ent[k]["bit_pos"]) + 48, 32)
    off = int(ent[0]["out_off"]) + 5  # block 0 cut at its head, block 1 whole
    n = int(ent[2]["out_off"]) - off
    with pytest.raises(native.BzhError) as e:
        dec.decode_range(damaged, trusting, off, n)
    assert e.value.status == -6 and "block CRC mismatch" in str(e.value) and "index entry 1 " in str(e.value), str(e.value)
    assert dec.decode_range(s, ent, 5, 20) == truth[5:25]  # the context goes on
    with pytest.raises(native.BzhError) as e:
        dec.decode_ranges(damaged, trusting, [(off, n)])
    assert e.value.status == -6 and "block CRC mismatch" in str(e.value) and "index entry 0 " in str(e.value), str(e.value)
    assert dec.decode_range(s, ent, 5, 20) == truth[5:25]
