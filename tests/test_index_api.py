"""CPU: random access into .bz2 without a device -- what the header declares, the span arithmetic of bzh_index_span on hand-made
indexes, BlockIndex's serialisation, the argument checks of the Python layer, the loud failure on a box without a GPU, and the
per-thread logic the kernels unrle_crc and unrle_walk_win share with a host build (tests/decode_host/unrle_host.cpp, compiled
with AddressSanitizer and UBSan) against a Python model of the expansion and of CRC-32/BZIP2."""
import bz2
import ctypes
import io
import os
import random
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import bz2_handbuilt, cases
from tests.golden import pymodel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("bzh_decode_index", "bzh_decode_index_device", "bzh_index_span", "bzh_decode_range", "bzh_decode_range_device")


def test_header_declares_random_access():
    text = open(os.path.join(ROOT, "include", "bzhip.h")).read()
    syms = set(re.findall(r"BZH_API[^;(]*?\b(bzh_\w+)\s*\(", text))
    for need in FUNCS:
        assert need in syms
    m = re.search(r"typedef struct \{([^}]*)\}\s*bzh_index_entry;", text)
    assert m, "bzh_index_entry is not declared"
    fields = re.findall(r"(uint64_t|uint32_t)\s+(\w+);", m.group(1))
    assert fields == [("uint64_t", "bit_pos"), ("uint64_t", "end_bit"), ("uint64_t", "out_off"), ("uint32_t", "out_len"),
                      ("uint32_t", "crc"), ("uint32_t", "stream"), ("uint32_t", "level")]
    # the header says what a range decode does not verify
    assert re.search(r"Stream CRCs are NOT verified", text) and "does not touch is not seen" in text


def test_bindings_mirror_the_header(native):
    assert native.MISSING == []
    for name in FUNCS:
        assert name in native.SIGNATURES
    assert ctypes.sizeof(native.IndexEntry) == 40 and native.INDEX_DTYPE.itemsize == 40
    for (name, ctype), field in zip(native.IndexEntry._fields_, native.INDEX_DTYPE.names):
        assert name == field and getattr(native.IndexEntry, name).offset == native.INDEX_DTYPE.fields[field][1]
    for attr in ("decode_index", "decode_range", "decode_range_device"):
        assert hasattr(native.Context, attr)
    import banzai_amd
    for name in ("build_index", "decompress_range", "BlockIndex", "IndexedReader"):
        assert name in banzai_amd.__all__ and hasattr(banzai_amd, name)


# ---- bzh_index_span --------------------------------------------------------------------------------------------------
def make_index(native, blocks, first_bit=32):
    """blocks: [(compressed bits, decoded bytes)] -> entries laid back to back from `first_bit`"""
    e = np.zeros(len(blocks), dtype=native.INDEX_DTYPE)
    bit, off = first_bit, 0
    for k, (bits, size) in enumerate(blocks):
        e[k] = (bit, bit + bits, off, size, 0x1000 + k, 0, 1)
        bit += bits
        off += size
    return e


def test_index_span(native):
    # block k: bits [32, 1000), [1000, 2008), [2008, 3001), [3001, 4000); bytes [0, 100), [100, 300), [300, 350), [350, 1350)
    e = make_index(native, [(968, 100), (1008, 200), (993, 50), (999, 1000)])
    span = lambda off, n: native.index_span(e, off, n)  # noqa: E731
    lo = [32 // 8, 1000 // 8, 2008 // 8, 3001 // 8]
    hi = [1000 // 8, 2008 // 8, (3001 + 7) // 8, (4000 + 7) // 8]
    assert hi == [125, 251, 376, 500]  # end_bit a multiple of 8 (1000, 2008, 4000) and not (3001): the byte that holds bit 3000 counts
    # inside one block
    assert span(0, 1) == (0, 1, lo[0], hi[0])
    assert span(10, 50) == (0, 1, lo[0], hi[0])
    assert span(150, 1) == (1, 2, lo[1], hi[1])
    assert span(349, 1) == (2, 3, lo[2], hi[2])
    assert span(350, 1000) == (3, 4, lo[3], hi[3])
    # ending exactly at a boundary, and one byte over it
    assert span(40, 60) == (0, 1, lo[0], hi[0])
    assert span(40, 61) == (0, 2, lo[0], hi[1])
    assert span(100, 200) == (1, 2, lo[1], hi[1])
    assert span(100, 201) == (1, 3, lo[1], hi[2])
    assert span(99, 1) == (0, 1, lo[0], hi[0])
    assert span(99, 2) == (0, 2, lo[0], hi[1])
    # three blocks, all four
    assert span(299, 52) == (1, 4, lo[1], hi[3])
    assert span(0, 1350) == (0, 4, lo[0], hi[3])
    # empty ranges: first == last, no bytes
    for off, n in ((0, 0), (100, 0), (1349, 0), (1350, 0), (1350, 10), (5000, 1), (2 ** 63, 2 ** 63)):
        first, last, blo, bhi = span(off, n)
        assert first == last and blo == bhi, (off, n)
    # clipped to the total
    assert span(1349, 1) == span(1349, 10 ** 12) == (3, 4, lo[3], hi[3])
    assert span(200, 2 ** 64 - 1) == (1, 4, lo[1], hi[3])
    assert span(0, 2 ** 64 - 1) == (0, 4, lo[0], hi[3])
    # no entries at all
    none = np.zeros(0, dtype=native.INDEX_DTYPE)
    assert native.index_span(none, 0, 0) == native.index_span(none, 0, 100) == native.index_span(none, 7, 1) == (0, 0, 0, 0)
    # one block whose end is mid-byte, and one that ends on a byte
    assert native.index_span(make_index(native, [(9, 5)], first_bit=80), 0, 5) == (0, 1, 10, 12)
    assert native.index_span(make_index(native, [(16, 5)], first_bit=80), 0, 5) == (0, 1, 10, 12)
    assert native.index_span(make_index(native, [(8, 5)], first_bit=80), 0, 5) == (0, 1, 10, 11)
    assert native.index_span(make_index(native, [(8, 5)], first_bit=83), 4, 1) == (0, 1, 10, 12)
    # the C function refuses null results
    z = ctypes.c_size_t(0)
    assert native.lib().bzh_index_span(None, 0, 0, 0, None, ctypes.byref(z), None, None) == -1
    # an index that does not start at offset 0 is not well formed (bzh_decode_range refuses it); the span of a range before its
    # first entry is empty (and no entry in front of the array is read to find that out)
    late = make_index(native, [(968, 10)], first_bit=80)
    late["out_off"] = 100
    for off, n in ((50, 10), (0, 100), (99, 1), (0, 1)):
        first, last, blo, bhi = native.index_span(late, off, n)
        assert first == last and blo == bhi == 0, (off, n)
    assert native.index_span(late, 95, 10) == native.index_span(late, 100, 10) == (0, 1, 10, 131)
    tail = make_index(native, [(968, 100), (1008, 200), (993, 50)])[1:]  # a slice of an index: offsets from 100
    assert native.index_span(tail, 0, 100)[:2] == (0, 0) and native.index_span(tail, 0, 101)[:2] == (0, 1)
    # a search, not a walk: agreement with a plain scan on a long random index
    rng = random.Random(5)
    big = make_index(native, [(rng.randrange(100, 5000), rng.randrange(1, 3000)) for _ in range(500)])
    ends = (big["out_off"] + big["out_len"]).tolist()
    for _ in range(300):
        off, n = rng.randrange(ends[-1] + 50), rng.randrange(0, 9000)
        stop = min(off + n, ends[-1])
        touched = [k for k in range(500) if int(big["out_off"][k]) < stop and ends[k] > off] if stop > off else []
        first, last, blo, bhi = native.index_span(big, off, n)
        assert list(range(first, last)) == touched
        if touched:
            assert (blo, bhi) == (int(big["bit_pos"][first]) // 8, (int(big["end_bit"][last - 1]) + 7) // 8)


# ---- BlockIndex ------------------------------------------------------------------------------------------------------
def test_block_index_round_trip_and_rejections(native):
    import banzai_amd
    e = make_index(native, [(968, 100), (1008, 200), (993, 50)])
    e["stream"] = [0, 0, 1]
    e["level"] = [9, 9, 3]
    ix = banzai_amd.BlockIndex(e, consumed=377)
    assert len(ix) == 3 and ix.size == 350 and ix.consumed == 377
    assert ix.span(99, 2) == native.index_span(e, 99, 2) == (0, 2, 4, 251)
    blob = ix.to_bytes()
    assert len(blob) == 32 + 3 * 40 and blob[32:] == e.tobytes()
    for form in (blob, bytearray(blob), memoryview(blob)):
        back = banzai_amd.BlockIndex.from_bytes(form)
        assert back.entries.tobytes() == e.tobytes() and back.size == 350 and back.consumed == 377 and len(back) == 3
    empty = banzai_amd.BlockIndex.from_bytes(banzai_amd.BlockIndex(e[:0], 14).to_bytes())
    assert len(empty) == 0 and empty.size == 0 and empty.consumed == 14 and empty.span(0, 10) == (0, 0, 0, 0)
    bad_magic = b"X" + blob[1:]
    bad_version = blob[:8] + struct.pack("<I", 2) + blob[12:]
    damaged = []
    for field, k, value in (("bit_pos", 1, 32), ("end_bit", 2, int(e["bit_pos"][2])), ("out_off", 2, 301), ("out_len", 0, 99),
                            ("level", 1, 0), ("level", 1, 10)):
        m = e.copy()
        m[field][k] = value
        damaged.append(blob[:32] + m.tobytes())
    for bad in [bad_magic, bad_version, blob[:-1], blob[:31], blob[:32 + 40], blob + b"\0", b""] + damaged:
        with pytest.raises(ValueError):
            banzai_amd.BlockIndex.from_bytes(bad)
    with pytest.raises(ValueError):
        banzai_amd.BlockIndex(np.frombuffer(damaged[0][32:], dtype=native.INDEX_DTYPE))


def test_python_surface_rejects_non_bytes(native):
    import banzai_amd
    ix = banzai_amd.BlockIndex(make_index(native, [(968, 100)]))
    for bad in ("text", 5, None, 3.5, ["x"]):
        with pytest.raises(TypeError):
            banzai_amd.build_index(bad)
        with pytest.raises(TypeError):
            banzai_amd.decompress_range(bad, ix, 0, 1)
        with pytest.raises(TypeError):
            banzai_amd.BlockIndex.from_bytes(bad)
        with pytest.raises(TypeError):
            banzai_amd.IndexedReader(bad, ix)
    for bad in (None, b"index", ix.entries, 7):
        with pytest.raises(TypeError):
            banzai_amd.decompress_range(b"BZh9", bad, 0, 1)
    for off, n in (("0", 1), (0, "1"), (0.0, 1), (0, None), (True, 1)):
        with pytest.raises(TypeError):
            banzai_amd.decompress_range(b"BZh9", ix, off, n)
    for off, n in ((-1, 1), (0, -1)):
        with pytest.raises(ValueError):
            banzai_amd.decompress_range(b"BZh9", ix, off, n)
    with pytest.raises(TypeError):
        banzai_amd.IndexedReader(b"BZh9", index=b"not an index")
    # a source shorter than the index says is an I/O error, before anything is decoded
    with pytest.raises(EOFError):
        banzai_amd.IndexedReader(io.BytesIO(b"BZh9" + bytes(50)), ix).read(5)
    # seek and tell are host arithmetic
    r = banzai_amd.IndexedReader(b"BZh9", ix)
    assert r.readable() and r.seekable() and not r.writable() and r.size == 100 and r.tell() == 0
    assert r.seek(40) == 40 and r.seek(5, io.SEEK_CUR) == 45 and r.seek(-10, io.SEEK_END) == 90 and r.tell() == 90
    assert r.seek(500) == 500 and r.read(10) == b"" and r.read() == b"" and r.readinto(bytearray(4)) == 0  # behind the end: nothing to decode
    assert r.seek(0, io.SEEK_END) == 100 and r.read(1) == b""
    with pytest.raises(ValueError):
        r.seek(-1)
    with pytest.raises(ValueError):
        r.seek(0, 3)
    with pytest.raises(TypeError):
        r.seek(1.5)


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(_have_gpu(), reason="only meaningful on a box without a GPU")
def test_no_gpu_fails_loudly(native):
    import banzai_amd
    s = bz2.compress(b"abc" * 100)
    with pytest.raises(native.BzhError) as e:
        banzai_amd.build_index(s)
    assert e.value.status == -3
    ix = banzai_amd.BlockIndex(make_index(native, [(len(s) * 8 - 32 - 80, 300)]))
    with pytest.raises(native.BzhError) as e:
        banzai_amd.decompress_range(s, ix, 0, 10)
    assert e.value.status == -3
    with pytest.raises(native.BzhError) as e:
        banzai_amd.IndexedReader(s)
    assert e.value.status == -3
    with pytest.raises(native.BzhError) as e:
        banzai_amd.IndexedReader(io.BytesIO(s), ix).read(5)
    assert e.value.status == -3


# ---- the shared per-thread logic, on the host ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def unrle_host(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed for the sanitizer build of the fold and clip logic"
    exe = str(tmp_path_factory.mktemp("unrle_host") / "unrle_host")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe,
                           os.path.join(ROOT, "tests", "decode_host", "unrle_host.cpp")])
    return exe


def run_blocks(exe, tmp_path, blocks):
    """-> [(crc, end state, expansion)] of unrle_host over `blocks`; a sanitizer report or a window that differs fails the run"""
    fin, fout = str(tmp_path / "blocks.bin"), str(tmp_path / "results.bin")
    with open(fin, "wb") as f:
        for b in blocks:
            f.write(struct.pack("<I", len(b)))
            f.write(b)
    p = subprocess.run([exe, fin, fout], capture_output=True, text=True)
    assert p.returncode == 0, f"unrle_host exit status {p.returncode}: {p.stderr[-3000:]}"
    blob = open(fout, "rb").read()
    res, at = [], 0
    for _ in blocks:
        crc, end, ln = struct.unpack_from("<III", blob, at)
        at += 12
        res.append((crc, end, blob[at:at + ln]))
        at += ln
    assert at == len(blob)
    return res


def check_blocks(exe, tmp_path, blocks):
    for b, (crc, end, got) in zip(blocks, run_blocks(exe, tmp_path, blocks)):
        want, closed = bz2_handbuilt.unrle(b)  # the Python model of the expansion
        assert got == want, (len(b), b[:40])
        assert (end != 4) == closed
        assert crc == pymodel.checksum(want), (len(b), b[:40])


def test_fold_and_clip_on_valid_blocks(unrle_host, tmp_path):
    """blocks as encoders cut them (pymodel.rle_one), short ones through every window: one tile, a ragged last tile, several
    tiles, runs of every length around the count byte, tiles that expand past the staging size"""
    blocks = []
    for d in cases.boundary_cases()[::7]:
        if d:
            blocks.append(d)
    for mode in ("text", "longruns", "shortruns", "same", "random"):
        for n in (1, 5, 17, 40, 4095, 4096, 4097, 12_345, 70_000):
            blocks.append(cases.gen(n, mode, 3))
    rle = []
    for raw in blocks:
        out, used = pymodel.rle_one(raw, 1)  # the first block an encoder cuts from it
        assert 0 < used <= len(raw)
        rle.append(bytes(out))
    for k in range(0, 12):  # runs of 0..11 and counts up to 255, a count byte equal to the run byte, a closing count of zero
        rle.append(b"ab" + b"z" * min(k, 4) + (bytes([k - 4]) if k >= 4 else b"") + b"c")
    rle += [b"q" * 4 + b"\xff", b"q" * 4 + b"\x00", b"\x05" * 5 + b"xyz", b"qrszzzz\x00", (b"aaaa\xff" + b"bbbb\xfe") * 2000,
            bytes(range(256)) * 40, b"x"]
    assert all(bz2_handbuilt.unrle(b)[1] for b in rle)
    check_blocks(unrle_host, tmp_path, rle)


def test_fold_and_clip_on_random_bytes(unrle_host, tmp_path):
    """any byte string is a block behind the inverse BWT to these kernels: random strings over a small alphabet (long runs,
    count bytes of every kind, blocks that end in state 4) and over all bytes, short enough for every window"""
    rng = random.Random(77)
    blocks = []
    for _ in range(700):
        n = rng.randrange(1, 40)
        stick = rng.randrange(4)
        alphabet = rng.choice([[0, 1, 2, 3, 9], [0, 1, 4, 5, 255], list(range(256))])
        b = bytearray()
        for i in range(n):
            b.append(b[-1] if i and rng.randrange(4) < stick else rng.choice(alphabet))
        blocks.append(bytes(b))
    for _ in range(6):  # several tiles of the same
        b = bytearray()
        for i in range(rng.randrange(5000, 13000)):
            b.append(b[-1] if i and rng.randrange(4) < 3 else rng.choice([0, 1, 4, 17, 255]))
        blocks.append(bytes(b))
    assert any(not bz2_handbuilt.unrle(b)[1] for b in blocks) and any(len(bz2_handbuilt.unrle(b)[0]) <= 48 for b in blocks)
    check_blocks(unrle_host, tmp_path, blocks)
