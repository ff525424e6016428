"""CPU: the surface of the encoder-side index -- bzh_encode_index_bound's arithmetic, the header and the ctypes table, the
argument checks of banzai_amd.encode_indexed, and the compiler's resource report for sync_emit.hip.  What needs a GPU is in
tests/test_gpu_encode_index.py; the rules of the kernel, as a serial model, in tests/test_esync_model.py."""
import ctypes
import io
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("bzh_encode_index", "bzh_encode_index_device", "bzh_encode_index_bound")


def test_header_and_bindings(native):
    text = open(os.path.join(ROOT, "include", "bzhip.h")).read()
    syms = set(re.findall(r"BZH_API[^;(]*?\b(bzh_\w+)\s*\(", text))
    L = ctypes.CDLL(native.LIB_PATH)
    for name in FUNCS:
        assert name in syms and name in native.SIGNATURES and hasattr(L, name), name
    assert native.MISSING == []
    # the two encode calls take bzh_encode[_device]'s arguments, then the interval and the two arrays of bzh_decode_index_sync
    for name, base in (("bzh_encode_index", "bzh_encode"), ("bzh_encode_index_device", "bzh_encode_device")):
        res, args = native.SIGNATURES[name]
        assert res is ctypes.c_int and args[:7] == native.SIGNATURES[base][1]
        assert args[7:] == [ctypes.c_uint32, native.idxp, ctypes.c_size_t, native.szp, native.syncp, ctypes.c_size_t, native.szp]


def test_bound_by_hand(native):
    """M = 100000 * level - 1; entries = n / (M * 4 / 5) + 2; points = entries * ((2000 * level - 1) / interval)"""
    # level 1: M * 4 / 5 = 399996 / 5 = 79999; 2000 groups
    assert native.encode_index_bound(1, 0, 256) == (2, 2 * 7)
    assert native.encode_index_bound(1, 79_998, 1) == (2, 2 * 1999)
    assert native.encode_index_bound(1, 79_999, 1) == (3, 3 * 1999)
    assert native.encode_index_bound(1, 1_000_000, 0) == (14, 0)          # 1,000,000 / 79,999 = 12
    assert native.encode_index_bound(1, 1_000_000, 1) == (14, 14 * 1999)
    assert native.encode_index_bound(1, 1_000_000, 256) == (14, 14 * 7)    # 1999 / 256 = 7
    assert native.encode_index_bound(1, 1_000_000, 32767) == (14, 0)
    # level 9: M * 4 / 5 = 3599996 / 5 = 719999; 18000 groups
    assert native.encode_index_bound(9, 100_000_000, 0) == (140, 0)       # 100,000,000 / 719,999 = 138
    assert native.encode_index_bound(9, 100_000_000, 1) == (140, 140 * 17999)
    assert native.encode_index_bound(9, 100_000_000, 256) == (140, 140 * 70)  # 17999 / 256 = 70
    assert native.encode_index_bound(9, 100_000_000, 32767) == (140, 0)
    assert native.encode_index_bound(9, 719_999 * 3 - 1, 17999) == (4, 4)


def test_bound_refuses(native):
    me, mp = ctypes.c_size_t(7), ctypes.c_size_t(7)
    f = native.lib().bzh_encode_index_bound
    for level, interval in ((0, 256), (10, 256), (-1, 1), (5, 32768), (5, 1 << 31)):
        assert f(level, 1000, interval, ctypes.byref(me), ctypes.byref(mp)) == -1, (level, interval)
        with pytest.raises(native.BzhError) as e:
            native.encode_index_bound(level, 1000, interval)
        assert e.value.status == -1
    assert f(5, 1000, 256, None, ctypes.byref(mp)) == -1 and f(5, 1000, 256, ctypes.byref(me), None) == -1
    assert (me.value, mp.value) == (7, 7)  # nothing written by a refused call
    assert f(5, 1000, 32767, ctypes.byref(me), ctypes.byref(mp)) == 0 and (me.value, mp.value) == (2, 0)


def test_entry_bound_covers_rle1s_worst_expansion(native, oracle):
    """runs of exactly four equal bytes: RLE1 writes five bytes for four, so a block takes the fewest raw bytes it can"""
    data = b"".join(bytes([k % 251]) * 4 for k in range(100_000))  # 400,000 bytes -> 500,000 RLE1 bytes
    _, blocks = oracle.encode(data, 1, want_blocks=True)
    assert len(blocks) == 6 and all(b.rle_len >= 99_998 for b in blocks[:-1])  # full blocks, and what the last cut left over
    assert min(b.in_len for b in blocks[:-1]) == 99_999 * 4 // 5  # the bound's divisor is the least a full block consumes
    max_e, max_p = native.encode_index_bound(1, len(data), 1)
    assert max_e >= len(blocks)
    assert max_p >= sum(((b.m + 49) // 50 - 1) for b in blocks)


def test_encode_indexed_argument_checks():
    import banzai_amd
    assert "encode_indexed" in banzai_amd.__all__
    src, out = io.BytesIO(b"abc"), io.BytesIO()
    for level in (0, 10, True, "9", None, 1.0):
        with pytest.raises(ValueError):
            banzai_amd.encode_indexed(src, out, level)
    for interval in (-1, 32768, 1 << 40):
        with pytest.raises(ValueError):
            banzai_amd.encode_indexed(src, out, 9, interval)
    for interval in ("256", 2.0, True, None):
        with pytest.raises(TypeError):
            banzai_amd.encode_indexed(src, out, 9, interval)

    class Text:
        def read(self):
            return "abc"
    with pytest.raises(TypeError):
        banzai_amd.encode_indexed(Text(), out, 9)
    assert src.tell() == 0 and out.getvalue() == b""  # nothing read, nothing written by a refused call


def test_sync_emit_uses_no_scratch_memory():
    """the compiler's resource report (scripts/resource_usage.py) for sync_emit.hip: both forms of the kernel, no spill, no
    scratch memory, LDS under 8 KB (one wavefront a point: the tile's bytes, 256 keys, two name tables, the point)"""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import resource_usage
    kernels = resource_usage.report(os.path.join(ROOT, "banzai_amd", "csrc", "sync_emit.hip"))
    emit = [r for r in kernels if "sync_emit" in r["name"]]
    assert len(emit) == 2, [r["name"] for r in kernels]
    for r in emit:
        assert r.get("ScratchSize [bytes/lane]", "0") == "0" and r.get("VGPRs Spill", "0") == "0" and r.get("SGPRs Spill", "0") == "0", r
        assert int(r["LDS Size [bytes/block]"]) <= 8 * 1024, r
