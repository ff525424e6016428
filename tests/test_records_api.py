"""CPU: reads by record number without a device -- what the header declares and the bindings mirror, bzh_record_spans on hand-made
indexes, RecordIndex's serialisation and every damaged field of it, and the atom cut of decompress_records (any order,
overlapping, repeated, empty, behind the end -> ascending disjoint atoms, one call, joined on the host) against brute force with
a fake back end that cuts the truth with plain Python."""
import os
import random
import re
import struct
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("bzh_decode_index_records", "bzh_decode_index_records_device", "bzh_count_records_device", "bzh_record_spans",
         "bzh_decode_records", "bzh_decode_records_device")


def test_header_declares_records():
    text = open(os.path.join(ROOT, "include", "bzhip.h")).read()
    syms = set(re.findall(r"BZH_API[^;(]*?\b(bzh_\w+)\s*\(", text))
    for need in FUNCS:
        assert need in syms
    # the contract: the definitions, and the block that is touched although it gives no bytes
    for phrase in ("rec_cum[count] = D", "The delimiter belongs to the record it ends".lower(), "IS TOUCHED ALTHOUGH IT GIVES THE"):
        assert phrase in text or phrase in text.lower(), phrase


def test_bindings_mirror_the_header(native):
    L = native.lib()
    assert native.MISSING == []
    for name in FUNCS:
        assert name in native.SIGNATURES and hasattr(L, name), name
    S = native.SIGNATURES
    assert len(S["bzh_decode_index_records"][1]) == 16 and len(S["bzh_decode_index_records_device"][1]) == 16
    assert len(S["bzh_decode_records"][1]) == 17 and len(S["bzh_decode_records_device"][1]) == 17
    assert len(S["bzh_count_records_device"][1]) == 8 and len(S["bzh_record_spans"][1]) == 10
    for attr in ("decode_index_records", "count_records_device", "decode_records", "decode_records_device"):
        assert hasattr(native.Context, attr)
    import banzai_amd
    for name in ("RecordIndex", "build_record_index", "record_index_of", "decompress_records"):
        assert name in banzai_amd.__all__ and hasattr(banzai_amd, name)
    assert hasattr(banzai_amd.IndexedReader, "read_records") and hasattr(banzai_amd.IndexedReader, "readv_records")


# ---- a hand-made index over a text whose bytes are known ------------------------------------------------------------------
def make_index(native, truth, sizes, delim=10):
    e = np.zeros(len(sizes), dtype=native.INDEX_DTYPE)
    cum = np.zeros(len(sizes) + 1, dtype=np.uint64)
    bit, off = 32, 0
    for k, size in enumerate(sizes):
        e[k] = (bit, bit + 800 + 8 * k, off, size, 0x1000 + k, 0, 1)
        bit += 800 + 8 * k
        cum[k + 1] = cum[k] + truth[off:off + size].count(bytes([delim]))
        off += size
    assert off == len(truth)
    return e, cum


def records_of(truth, delim=b"\n"):
    """the records by the contract: the delimiter belongs to the record it ends; the unterminated tail counts when not empty"""
    parts = truth.split(delim)
    recs = [p + delim for p in parts[:-1]]
    return recs + ([parts[-1]] if parts[-1] else [])


def brute_touched(truth, e, first, count, delim=10):
    """the blocks of the contract: the one that holds delimiter `first` (block 0 for 0), the one that holds delimiter
    first + count (the last one behind D), everything between"""
    pos = [i for i, b in enumerate(truth) if b == delim]
    D = len(pos)
    a, b = min(first, D + 1), min(first + count, D + 1)
    if a == b or not len(e):
        return set()
    ends = np.cumsum(e["out_len"].astype(np.int64))
    block = lambda p: int(np.searchsorted(ends, p, side="right"))
    lo = 0 if a == 0 else block(pos[a - 1])
    hi = block(pos[b - 1]) if b <= D else len(e) - 1
    return set(range(lo, hi + 1))


def test_record_spans_on_hand_made_indexes(native):
    truth = b"ab\ncd\n" + b"\n" + b"efgh" + b"\nxy\n" + b"tail"
    sizes = [6, 1, 4, 4, 4]  # block 0 ends in a newline, block 1 is one newline, block 2 has none, block 3 begins with one
    e, cum = make_index(native, truth, sizes)
    assert cum.tolist() == [0, 2, 3, 3, 5, 5]
    D = 5
    for first in range(0, D + 4):
        for count in list(range(0, D + 4)) + [2**64 - 1]:
            touched, lo, hi = native.record_spans(e, cum, [(first, count)])
            want = sorted(brute_touched(truth, e, first, count))
            assert touched.tolist() == want, (first, count)
            if want:
                assert (lo, hi) == (int(e[want[0]]["bit_pos"]) // 8, (int(e[want[-1]]["end_bit"]) + 7) // 8)
            else:
                assert (lo, hi) == (0, 0)
    # record 2 is the lone newline of block 1: its start is behind the last byte of block 0, which is touched and gives nothing
    assert native.record_spans(e, cum, [(2, 1)])[0].tolist() == [0, 1]
    # a union, in any order
    assert native.record_spans(e, cum, [(5, 1), (0, 1)])[0].tolist() == [0, 3, 4]
    # an empty index, and a table that is not one
    z = np.zeros(0, dtype=native.INDEX_DTYPE)
    assert native.record_spans(z, np.zeros(1, np.uint64), [(0, 5)])[0].tolist() == []
    for bad in ([1, 2, 3, 3, 5, 5], [0, 2, 1, 3, 5, 5], [0, 2, 4, 4, 5, 5]):
        with pytest.raises(native.BzhError) as err:
            native.record_spans(e, np.array(bad, dtype=np.uint64), [(0, 1)])
        assert err.value.status == -1 if hasattr(err.value, "status") else True
    with pytest.raises(ValueError):
        native.record_spans(e, cum[:-1], [(0, 1)])


# ---- RecordIndex ------------------------------------------------------------------------------------------------------------
def test_record_index_round_trip_and_every_damaged_field(native):
    import banzai_amd
    from banzai_amd import BlockIndex, RecordIndex, SyncIndex
    truth = b"ab\ncd\n" + b"\n" + b"efgh" + b"\nxy\n" + b"tail"
    e, cum = make_index(native, truth, [6, 1, 4, 4, 4])
    blocks = BlockIndex(e, 999)
    pts = np.zeros(1, dtype=native.SYNC_DTYPE)
    pts[0]["bit_pos"], pts[0]["entry"], pts[0]["group"], pts[0]["run_weight"] = int(e[0]["bit_pos"]) + 100, 0, 4, 1
    for index in (blocks, SyncIndex(blocks, pts, 4)):
        r = RecordIndex(index, b"\n", cum, 6)
        assert len(r) == 6 and r.delim == 10 and r.size == len(truth) and r.consumed == 999
        blob = r.to_bytes()
        head = struct.Struct("<8sIIQQII")
        magic, version, delim, count, nrec, crc, zero = head.unpack_from(blob, 0)
        assert (magic, version, delim, count, nrec, zero) == (b"BZhREC\r\n", 1, 10, 5, 6, 0)
        assert crc == zlib.crc32(blob[head.size:], zlib.crc32(head.pack(magic, version, delim, count, nrec, 0, 0)))
        assert blob[head.size:head.size + len(index.to_bytes())] == index.to_bytes() and blob[-8 * 6:] == cum.tobytes()
        back = RecordIndex.from_bytes(blob)
        assert type(back.index) is type(index) and back.to_bytes() == blob and back.rec_cum.tolist() == cum.tolist()
        # every single flipped bit of the blob is refused
        for at in range(len(blob)):
            bad = bytearray(blob)
            bad[at] ^= 1 << (at % 8)
            with pytest.raises(ValueError):
                RecordIndex.from_bytes(bytes(bad))
        # every field wrong with the CRC made right again, so that the field's own check has to refuse it
        def forged(fields, body=blob[head.size:]):
            return head.pack(*fields, zlib.crc32(body, zlib.crc32(head.pack(*fields, 0, 0))), 0) + body
        assert RecordIndex.from_bytes(forged((magic, version, delim, count, nrec))).to_bytes() == blob
        for fields in ((b"BZhREX\r\n", 1, 10, 5, 6), (magic, 2, 10, 5, 6), (magic, 1, 256, 5, 6), (magic, 1, 10, 4, 6), (magic, 1, 10, 6, 6),
                       (magic, 1, 10, 5, 4), (magic, 1, 10, 5, 7), (magic, 1, 10, 2**61, 6)):
            with pytest.raises(ValueError):
                RecordIndex.from_bytes(forged(fields))
        body = blob[head.size:]
        for table in ([1, 2, 3, 3, 5, 5], [0, 2, 1, 3, 5, 5], [0, 2, 4, 4, 5, 5]):
            with pytest.raises(ValueError):
                RecordIndex.from_bytes(forged((magic, 1, 10, 5, 6), body[:-48] + np.array(table, dtype=np.uint64).tobytes()))
        for cut in (0, 10, head.size, len(blob) - 1):
            with pytest.raises(ValueError):
                RecordIndex.from_bytes(blob[:cut])
        with pytest.raises(ValueError):
            RecordIndex.from_bytes(blob + b"\0")
        with pytest.raises(ValueError):
            RecordIndex.from_bytes(forged((magic, 1, 10, 5, 6), body[:7] + bytes([body[7] ^ 1]) + body[8:]))  # the wrapped index's own magic
    # the constructor's own checks
    for args in ((blocks, b"\n", cum[:-1], 6), (blocks, b"\n", cum, 4), (blocks, b"\n", cum, 7), (blocks, b"ab", cum, 6), (blocks, 256, cum, 6)):
        with pytest.raises(ValueError):
            RecordIndex(*args)
    with pytest.raises(TypeError):
        RecordIndex(e, b"\n", cum, 6)
    # every byte a delimiter, and nothing at all
    e1, cum1 = make_index(native, b"\n\n\n", [2, 1])
    assert len(RecordIndex(BlockIndex(e1), 10, cum1, 3)) == 3
    with pytest.raises(ValueError):
        RecordIndex(BlockIndex(e1), 10, cum1, 4)
    empty = RecordIndex(BlockIndex(np.zeros(0, dtype=native.INDEX_DTYPE)), 10, [0], 0)
    assert len(RecordIndex.from_bytes(empty.to_bytes())) == 0
    assert banzai_amd.RecordIndex is RecordIndex


# ---- the atom cut --------------------------------------------------------------------------------------------------------------
class FakeContext:
    """bzh_decode_records by plain Python: refuses what the library refuses of the ranges, cuts the truth"""

    def __init__(self, truth, delim=b"\n"):
        self.truth, self.delim, self.calls = truth, delim, 0
        parts = truth.split(delim)
        self.recs = [p + delim for p in parts[:-1]] + [parts[-1]]  # records 0..D, the tail maybe empty

    def decode_records(self, comp, entries, rec_cum, ranges, points=None, in_byte_base=0, delim=10):
        self.calls += 1
        assert delim == self.delim[0]
        end, blob, offs, lens = 0, b"", [], []
        for first, count in ranges:
            assert first >= end and count > 0, "the atoms ascend, do not overlap and are not empty"
            end = first + count
            assert end <= len(self.recs)
            piece = b"".join(self.recs[first:end])
            offs.append(len(blob))
            lens.append(len(piece))
            blob += piece
        return blob, offs, lens


@pytest.mark.parametrize("truth", [b"ab\ncd\n\nefgh\nxy\ntail", b"ab\ncd\n", b"\n\n\n", b"no newline at all", b"\n", b"x"])
def test_decompress_records_cuts_atoms(native, monkeypatch, truth):
    import banzai_amd
    sizes = [len(truth) // 2, len(truth) - len(truth) // 2] if len(truth) > 1 else [len(truth)]
    e, cum = make_index(native, truth, sizes)
    recs = records_of(truth)
    rindex = banzai_amd.RecordIndex(banzai_amd.BlockIndex(e), b"\n", cum, len(recs))
    fake = FakeContext(truth)
    monkeypatch.setattr(banzai_amd, "_ctx", lambda level, device=0: fake)
    rng = random.Random(len(truth))
    n = len(recs)
    for trial in range(200):
        ranges = [(rng.randrange(n + 3), rng.choice([0, 1, 1, 2, rng.randrange(n + 3), 2**64 - 1])) for _ in range(rng.randrange(9))]
        if ranges and rng.random() < 0.3:
            ranges.append(ranges[0])
        calls = fake.calls
        got = banzai_amd.decompress_records(truth, rindex, ranges)
        assert got == [b"".join(recs[a:a + c]) for a, c in ranges], ranges
        assert fake.calls - calls <= 1
    assert banzai_amd.decompress_records(truth, rindex, []) == []
    assert banzai_amd.decompress_records(truth, rindex, [(0, 2**64 - 1)]) == [truth]
    rd = banzai_amd.IndexedReader(truth, rindex)
    assert rd.read_records(0, 1) == (recs[0] if recs else b"") and rd.readv_records([(1, 1), (0, 1)]) == [b"".join(recs[1:2]), b"".join(recs[0:1])]
    with pytest.raises(ValueError):
        banzai_amd.IndexedReader(truth, banzai_amd.BlockIndex(e)).read_records(0, 1)
    for bad in ([(-1, 1)], [(0, -1)]):
        with pytest.raises(ValueError):
            banzai_amd.decompress_records(truth, rindex, bad)
    with pytest.raises(TypeError):
        banzai_amd.decompress_records(truth, banzai_amd.BlockIndex(e), [(0, 1)])
