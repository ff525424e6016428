"""CPU: the surface of the sync points -- the header and the ctypes table, the 288-byte point, SyncIndex and its byte format,
and the compiler's resource report for decode.hip (no kernel of it may use scratch memory or spill).  What needs a GPU is in
tests/test_gpu_sync.py; the shared decode logic under sanitizers in tests/test_sync_host.py."""
import bz2
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from tests import sync_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("bzh_decode_index_sync", "bzh_decode_index_sync_device", "bzh_decode_range_sync", "bzh_decode_range_sync_device")


def test_header_and_bindings(native):
    text = open(os.path.join(ROOT, "include", "bzhip.h")).read()
    syms = set(re.findall(r"BZH_API[^;(]*?\b(bzh_\w+)\s*\(", text))
    L = ctypes.CDLL(native.LIB_PATH)
    for name in FUNCS:
        assert name in syms and name in native.SIGNATURES and hasattr(L, name), name
    assert native.MISSING == []
    assert native.SYNC_DTYPE == sync_model.POINT_DTYPE and native.SYNC_DTYPE.itemsize == ctypes.sizeof(native.SyncPoint) == 288
    for name, (offset, size) in {"bit_pos": (0, 8), "entry": (8, 4), "group": (12, 4), "out_pos": (16, 4), "run": (20, 4),
                                 "run_weight": (24, 4), "reserved": (28, 4), "mtf": (32, 256)}.items():
        f = getattr(native.SyncPoint, name)
        assert (f.offset, f.size) == (offset, size) and native.SYNC_DTYPE.fields[name][1] == offset, name
    m = re.search(r"typedef struct \{([^}]*)\} bzh_sync_point;", text)
    assert m and re.findall(r"(\w+)(?:\[256\])?;", m.group(1)) == ["bit_pos", "entry", "group", "out_pos", "run", "run_weight",
                                                                    "reserved", "mtf"]


@pytest.fixture(scope="module")
def model_index(native, tmp_path_factory):
    """a SyncIndex without a GPU: the host model's blocks and points of a two-stream input at interval 3 (out_len is the size of
    the last column there, which is as good as any for the byte format)"""
    import banzai_amd
    tmp = tmp_path_factory.mktemp("sync_api")
    exe = sync_model.build(tmp)
    s = bz2.compress(bytes(range(256)) * 40 + b"sync points " * 900, 1) + bz2.compress(b"the second stream " * 700, 9)
    res, _ = sync_model.run(exe, tmp, [s], 3)
    blocks, pts, _, ents = res[0]
    assert blocks == 2 and len(pts) >= 4 and set(pts["entry"].tolist()) == {0, 1}
    e = np.zeros(blocks, dtype=native.INDEX_DTYPE)
    off = 0
    for k, (bit_pos, end_bit, size, crc, stream, level) in enumerate(ents):
        e[k] = (bit_pos, end_bit, off, size, crc, stream, level)
        off += size
    return banzai_amd.SyncIndex(banzai_amd.BlockIndex(e, len(s)), pts, 3)


def test_sync_index_round_trip(native, model_index):
    import banzai_amd
    ix = model_index
    blob = ix.to_bytes()
    back = banzai_amd.SyncIndex.from_bytes(blob)
    assert back.interval == 3 and back.points.tobytes() == ix.points.tobytes() and back.points.dtype == native.SYNC_DTYPE
    assert back.blocks.entries.tobytes() == ix.blocks.entries.tobytes() and back.blocks.consumed == ix.blocks.consumed
    assert back.to_bytes() == blob and banzai_amd.SyncIndex.from_bytes(bytearray(blob)).to_bytes() == blob
    assert (back.size, back.consumed, len(back)) == (ix.blocks.size, ix.blocks.consumed, 2) and back.span(0, 10) == ix.blocks.span(0, 10)
    # the BlockIndex inside serialises to the bytes it always had: its version-1 format, found whole inside the blob
    inner = ix.blocks.to_bytes()
    assert inner == banzai_amd.BlockIndex(ix.blocks.entries, ix.blocks.consumed).to_bytes()
    assert inner[:8] == banzai_amd.BlockIndex.MAGIC and len(inner) == 32 + 40 * 2
    head = banzai_amd.SyncIndex._HEAD.size
    assert blob[:8] == banzai_amd.SyncIndex.MAGIC != banzai_amd.BlockIndex.MAGIC
    assert blob[head:head + len(inner)] == inner and len(blob) == head + len(inner) + 288 * len(ix.points)
    with pytest.raises(ValueError):
        banzai_amd.BlockIndex.from_bytes(blob)  # the two formats do not pass for each other
    with pytest.raises(ValueError):
        banzai_amd.SyncIndex.from_bytes(inner)


def test_sync_index_refuses_damaged_blobs(model_index):
    import banzai_amd
    blob = model_index.to_bytes()
    for n in range(len(blob)):  # every truncation
        with pytest.raises(ValueError):
            banzai_amd.SyncIndex.from_bytes(blob[:n])
    for extra in (b"\0", b"\xff", bytes(288), bytes(40), blob):  # extended
        with pytest.raises(ValueError):
            banzai_amd.SyncIndex.from_bytes(blob + extra)
    m = bytearray(blob)
    for bit in range(len(blob) * 8):  # every single-bit flip
        m[bit // 8] ^= 1 << (bit % 8)
        with pytest.raises(ValueError):
            banzai_amd.SyncIndex.from_bytes(m)
        m[bit // 8] ^= 1 << (bit % 8)
    assert bytes(m) == blob


def test_sync_index_refuses_ill_formed_points(native, model_index):
    """the constructor applies bzh_decode_range_sync's rule for ill-formed points (one case per clause)"""
    import banzai_amd
    ix = model_index
    second = int(np.flatnonzero(ix.points["entry"] == 1)[0])
    assert second >= 2
    cases = [("reserved", 0, 1), ("group", 0, 0), ("group", 1, 32767), ("entry", 0, 2), ("entry", 0, 1),
             ("group", 1, int(ix.points["group"][0])), ("bit_pos", 0, int(ix.blocks.entries["bit_pos"][0])),
             ("bit_pos", 0, int(ix.blocks.entries["end_bit"][0])), ("bit_pos", 1, int(ix.points["bit_pos"][0])),
             ("out_pos", 1, int(ix.points["out_pos"][0]) - 1), ("out_pos", second - 1, 100_001), ("run_weight", 0, 0),
             ("run_weight", 0, 3), ("run_weight", 0, 1 << 23), ("run", 0, 1)]
    for field, k, value in cases:
        bad = ix.points.copy()
        if field == "run":
            bad["run_weight"][k] = 1  # no digit pending, yet a run
        bad[field][k] = value
        with pytest.raises(ValueError):
            banzai_amd.SyncIndex(ix.blocks, bad, 3)
    for interval in (0, 32768):
        with pytest.raises(ValueError):
            banzai_amd.SyncIndex(ix.blocks, ix.points, interval)
    with pytest.raises(TypeError):
        banzai_amd.SyncIndex(ix.blocks.entries, ix.points, 3)
    pending = ix.points.copy()  # a pending run of three digits: run + 1 in [8, 15]
    pending["run_weight"][0], pending["run"][0] = 8, 7
    assert banzai_amd.SyncIndex(ix.blocks, pending, 3).points["run"][0] == 7


def test_python_surface_argument_checks(native, model_index):
    import banzai_amd
    for bad in (0, 32768, -1):
        with pytest.raises(ValueError):
            banzai_amd.build_sync_index(b"BZh9", bad)
    for bad in ("256", 2.0, True, None):
        with pytest.raises(TypeError):
            banzai_amd.build_sync_index(b"BZh9", bad)
    with pytest.raises(TypeError):
        banzai_amd.build_sync_index("BZh9")
    with pytest.raises(TypeError):
        banzai_amd.decompress_range(b"", model_index.points, 0, 1)
    with pytest.raises(TypeError):
        banzai_amd.IndexedReader(b"", model_index.points)
    assert banzai_amd.IndexedReader(b"", model_index).size == model_index.size  # accepted wherever a BlockIndex is


def test_no_decode_kernel_uses_scratch_memory():
    """the compiler's own resource report (scripts/resource_usage.py) for decode.hip: no kernel spills a register or uses
    scratch memory, and the segment kernel keeps its LDS at the 16,744 bytes of its tables (BzdWork, for one wavefront a
    block: 51 KB)"""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import resource_usage
    kernels = resource_usage.report(os.path.join(ROOT, "banzai_amd", "csrc", "decode.hip"))
    names = " ".join(r["name"] for r in kernels)
    for need in ("decode_block_kernel", "decode_block_sync_kernel", "decode_header_kernel", "decode_segment_kernel", "unrle_walk_win"):
        assert need in names, need
    bad = [(r["name"], r.get("VGPRs Spill"), r.get("SGPRs Spill"), r.get("ScratchSize [bytes/lane]")) for r in kernels
           if r.get("ScratchSize [bytes/lane]", "0") != "0" or r.get("VGPRs Spill", "0") != "0" or r.get("SGPRs Spill", "0") != "0"]
    assert not bad, bad
    seg = [r for r in kernels if "decode_segment_kernel" in r["name"]]
    assert len(seg) == 1 and int(seg[0]["LDS Size [bytes/block]"]) <= 17 * 1024
