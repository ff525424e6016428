"""CPU: the surface of the streaming index and of the index files of the C ABI -- the header, the exports and the ctypes table for
bzh_stream_begin_index / _index_pending / _index_take and bzh_index_blob_size / _write / _read; the blobs against the Python
classes that defined the formats (BlockIndex.to_bytes, SyncIndex.to_bytes), byte for byte and both ways; damaged blobs against
both readers; the argument checks of banzai_amd.encode_indexed_stream.  The blob calls are pure host code.  What needs a GPU is
in tests/test_gpu_stream_index.py and tests/test_gpu_cli_index.py; the same functions under sanitizers in
tests/test_stream_index_host.py."""
import ctypes
import io
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("bzh_stream_begin_index", "bzh_stream_index_pending", "bzh_stream_index_take", "bzh_index_blob_size", "bzh_index_blob_write",
         "bzh_index_blob_read")


def test_header_and_bindings(native):
    text = open(os.path.join(ROOT, "include", "bzhip.h")).read()
    syms = set(re.findall(r"BZH_API[^;(]*?\b(bzh_\w+)\s*\(", text))
    L = ctypes.CDLL(native.LIB_PATH)
    for name in FUNCS:
        assert name in syms and name in native.SIGNATURES and hasattr(L, name), name
    assert native.MISSING == []
    S = native.SIGNATURES
    assert S["bzh_stream_begin_index"] == (ctypes.c_int, S["bzh_stream_begin"][1] + [ctypes.c_uint32])
    # the take hands out the two arrays as bzh_decode_index_sync does
    assert S["bzh_stream_index_take"][1][1:] == S["bzh_decode_index_sync"][1][4:10]
    assert S["bzh_index_blob_size"][0] is ctypes.c_size_t
    for m in ("stream_begin_index", "stream_index_pending", "stream_index_take"):
        assert callable(getattr(native.Context, m))


def seeded_index(native, seed, count, npts, level=9):
    """well-formed arrays: blocks of 174 to 7,000,000 bits back to back from bit 32, points spread over the blocks in order"""
    rng = np.random.default_rng(seed)
    e = np.zeros(count, dtype=native.INDEX_DTYPE)
    bits = rng.integers(174, 7_000_000, count, dtype=np.uint64)
    ends = np.uint64(32) + np.cumsum(bits, dtype=np.uint64)
    e["end_bit"] = ends
    e["bit_pos"] = ends - bits
    e["out_len"] = rng.integers(1, 100_000 * level, count)
    e["out_off"] = np.concatenate([np.zeros(1, np.uint64), np.cumsum(e["out_len"][:-1], dtype=np.uint64)]) if count else 0
    e["crc"] = rng.integers(0, 1 << 32, count, dtype=np.uint64)
    e["level"] = level
    p = np.zeros(npts if count else 0, dtype=native.SYNC_DTYPE)
    if p.size:
        p["entry"] = np.sort(rng.integers(0, count, p.size))
        for k in range(count):
            own = np.flatnonzero(p["entry"] == k)
            # at most 32766 groups and one bit apart at the least
            own = own[:min(own.size, 32766, int(bits[k]) - 2)]
            p["group"][own] = 1 + np.arange(own.size)
            p["bit_pos"][own] = e["bit_pos"][k] + np.uint64(1) + np.arange(own.size, dtype=np.uint64)
            p["out_pos"][own] = np.arange(own.size)
        p = p[p["group"] > 0]
        p["run_weight"] = 1 << rng.integers(0, 23, p.size)
        p["run"] = p["run_weight"] - 1 + rng.integers(0, 1 << 22, p.size) % p["run_weight"]
        p["mtf"] = rng.integers(0, 256, (p.size, 256))
    return e, p


CASES = [(0, 0), (1, 0), (1, 3), (300, 0), (300, 4000), (7, 2500)]


@pytest.mark.parametrize("count,npts", CASES)
@pytest.mark.parametrize("interval", [0, 1, 256])
def test_blobs_are_the_python_classes_blobs(native, count, npts, interval):
    """bzh_index_blob_write == BlockIndex / SyncIndex .to_bytes(), and bzh_index_blob_read of those gives the arrays back"""
    import banzai_amd
    e, p = seeded_index(native, 1000 * count + npts + interval, count, npts if interval else 0)
    consumed = 12345 + count
    blocks = banzai_amd.BlockIndex(e, consumed)
    want = banzai_amd.SyncIndex(blocks, p, interval).to_bytes() if interval else blocks.to_bytes()
    got = native.index_blob_write(e, p, interval, consumed)
    assert got == want
    assert native.lib().bzh_index_blob_size(e.size, p.size, interval) == len(want)
    re_, rp, riv, rcons = native.index_blob_read(want)
    assert (riv, rcons) == (interval, consumed)
    assert re_.tobytes() == e.tobytes() and rp.tobytes() == p.tobytes()
    # and the Python reader takes the C writer's blob
    back = (banzai_amd.SyncIndex if interval else banzai_amd.BlockIndex).from_bytes(got)
    assert back.to_bytes() == want and back.consumed == consumed


def test_cap_sets_both_counts(native):
    import banzai_amd
    e, p = seeded_index(native, 5, 9, 40)
    blob = banzai_amd.SyncIndex(banzai_amd.BlockIndex(e, 77), p, 16).to_bytes()
    for me, mp in ((0, 0), (e.size - 1, p.size), (e.size, p.size - 1), (0, p.size), (e.size, 0)):
        st, _, _, cnt, npts, iv, cons = native.index_blob_read_raw(blob, me, mp)
        assert (st, cnt, npts, iv, cons) == (-4, e.size, p.size, 16, 77), (me, mp)
    st, re_, rp, cnt, npts, _, _ = native.index_blob_read_raw(blob, e.size + 3, p.size + 3)
    assert st == 0 and re_.tobytes() == e.tobytes() and rp.tobytes() == p.tobytes()
    # the writer: a buffer one byte short names the size
    out = np.zeros(len(blob), np.uint8)
    olen = ctypes.c_size_t(0)
    _, ep = native._entries(e)
    _, pp = native._points(p)
    f = native.lib().bzh_index_blob_write
    assert f(ep, e.size, pp, p.size, 16, 77, native.ptr(out), len(blob) - 1, ctypes.byref(olen)) == -4 and olen.value == len(blob)
    assert f(ep, e.size, pp, p.size, 16, 77, native.ptr(out), len(blob), ctypes.byref(olen)) == 0 and out.tobytes() == blob


def test_write_and_read_refuse_bad_arguments(native):
    e, p = seeded_index(native, 6, 2, 3)
    L = native.lib()
    assert L.bzh_index_blob_size(2, 3, 0) == 0 and L.bzh_index_blob_size(2, 3, 32768) == 0
    assert L.bzh_index_blob_size(2, 3, 32767) == 40 + 32 + 80 + 3 * 288
    for interval in (0, 32768):  # points without an interval; an interval above 32767
        with pytest.raises(native.BzhError) as err:
            native.index_blob_write(e, p, interval, 0)
        assert err.value.status == -1
    cnt, npts, iv, cons = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_uint32(0), ctypes.c_uint64(0)
    blob = np.frombuffer(native.index_blob_write(e, None, 0, 0), dtype=np.uint8)
    args = [native.ptr(blob), blob.size, None, 0, ctypes.byref(cnt), None, 0, ctypes.byref(npts), ctypes.byref(iv), ctypes.byref(cons)]
    assert L.bzh_index_blob_read(*args) == -4 and cnt.value == 2
    for k in (0, 4, 7, 8, 9):
        bad = list(args)
        bad[k] = None
        assert L.bzh_index_blob_read(*bad) == -1, k
    bad = list(args)
    bad[3] = 2  # room claimed, no array
    assert L.bzh_index_blob_read(*bad) == -1


def test_both_readers_refuse_damaged_sync_blobs(native):
    """every truncation of a small blob, every bit of its header and a sample of its body flipped: status -6 from the C
    reader, ValueError from SyncIndex.from_bytes -- the CRC covers everything"""
    import banzai_amd
    e, p = seeded_index(native, 7, 2, 2)
    blob = banzai_amd.SyncIndex(banzai_amd.BlockIndex(e, 4242), p, 256).to_bytes()
    assert len(blob) == 40 + 32 + 80 + 576

    def refused(b):
        st = native.index_blob_read_raw(b, 16, 16)[0]
        try:
            banzai_amd.SyncIndex.from_bytes(b)
            py = False
        except ValueError:
            py = True
        return st == -6 and py

    assert not refused(blob)
    for cut in range(len(blob)):
        assert refused(blob[:cut]), cut
    assert refused(blob + b"\0")
    rng = np.random.default_rng(11)
    bits = list(range(40 * 8)) + sorted(set(rng.integers(40 * 8, len(blob) * 8, 400).tolist()))
    for bit in bits:
        b = bytearray(blob)
        b[bit // 8] ^= 1 << (bit % 8)
        assert refused(bytes(b)), bit


def test_both_readers_refuse_damaged_block_blobs(native):
    """a block index blob has no CRC (BlockIndex.to_bytes defined it so): both readers refuse every truncation, a byte too many, a
    wrong magic, version or count; the C reader also a non-zero reserved field.  Damage inside the entries is the decode calls'
    to find: they check every entry they use against the bytes"""
    import banzai_amd
    e, _ = seeded_index(native, 8, 3, 0)
    blob = banzai_amd.BlockIndex(e, 999).to_bytes()

    def status(b):
        return native.index_blob_read_raw(b, 16, 0)[0]

    def py_refuses(b):
        try:
            banzai_amd.BlockIndex.from_bytes(b)
            return False
        except ValueError:
            return True

    assert status(blob) == 0 and not py_refuses(blob)
    for cut in range(len(blob)):
        assert status(blob[:cut]) == -6 and py_refuses(blob[:cut]), cut
    assert status(blob + b"\0") == -6 and py_refuses(blob + b"\0")
    for bit in list(range(12 * 8)) + list(range(16 * 8, 24 * 8)):  # magic, version, count
        b = bytearray(blob)
        b[bit // 8] ^= 1 << (bit % 8)
        assert status(bytes(b)) == -6 and py_refuses(bytes(b)), bit
    for bit in range(12 * 8, 16 * 8):  # reserved
        b = bytearray(blob)
        b[bit // 8] ^= 1 << (bit % 8)
        assert status(bytes(b)) == -6, bit
    # one kind's reader is not the other's
    assert py_refuses(banzai_amd.SyncIndex(banzai_amd.BlockIndex(e, 1), np.zeros(0, native.SYNC_DTYPE), 5).to_bytes())


def test_encode_indexed_stream_argument_checks():
    import banzai_amd
    assert "encode_indexed_stream" in banzai_amd.__all__
    src, out = io.BytesIO(b"abc"), io.BytesIO()
    for level in (0, 10, True, "9", None, 1.0):
        with pytest.raises(ValueError):
            banzai_amd.encode_indexed_stream(src, out, level)
    for interval in (-1, 32768, 1 << 40):
        with pytest.raises(ValueError):
            banzai_amd.encode_indexed_stream(src, out, 9, interval)
    for interval in ("256", 2.0, True, None):
        with pytest.raises(TypeError):
            banzai_amd.encode_indexed_stream(src, out, 9, interval)
    for chunk in (0, -5):
        with pytest.raises(ValueError):
            banzai_amd.encode_indexed_stream(src, out, 9, 256, chunk)
    for chunk in ("1", 2.0, True, None):
        with pytest.raises(TypeError):
            banzai_amd.encode_indexed_stream(src, out, 9, 256, chunk)
    assert src.tell() == 0 and out.getvalue() == b""  # nothing read, nothing written by a refused call
