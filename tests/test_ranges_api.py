"""CPU: what a call over many ranges does before it reaches the device -- banzai_amd._subindex, the index of the touched blocks
alone that IndexedReader.readv hands over with only their compressed bytes, on synthetic indexes; bzh_index_spans through its
binding; and the argument errors of the new entry points that need no device."""
import ctypes
import random

import numpy as np
import pytest

U64 = 2**64 - 1


def synthetic(rng, blocks, with_points):
    """an index of `blocks` blocks of 1 to 400 bytes in up to three streams, neighbours sharing a byte or not, and (with_points)
    0 to 4 sync points inside each -> BlockIndex or SyncIndex"""
    import banzai_amd
    from banzai_amd import _native
    e = np.zeros(blocks, dtype=_native.INDEX_DTYPE)
    pts = []
    bit, off = 32, 0
    for k in range(blocks):
        bits = rng.randrange(174, 3000)
        n = rng.choice((1, rng.randrange(1, 401)))
        e[k] = (bit, bit + bits, off, n, rng.getrandbits(32), k * 3 // max(blocks, 1), rng.randrange(1, 10))
        cuts = sorted(rng.sample(range(bit + 1, bit + bits), rng.randrange(0, 5))) if with_points else []
        for g, b in enumerate(cuts):
            pts.append((b, k, g + 1, g, 0, 1, 0, np.zeros(256, np.uint8)))
        bit += bits + rng.choice((0, 0, 81, 8 * rng.randrange(11, 500) + rng.randrange(8)))
        off += n
    index = banzai_amd.BlockIndex(e, (bit + 7) // 8 + 10)
    if with_points:
        index = banzai_amd.SyncIndex(index, np.array(pts, dtype=_native.SYNC_DTYPE) if pts else np.zeros(0, _native.SYNC_DTYPE), 4)
    return index


def random_ranges(rng, total, n):
    out = []
    for _ in range(n):
        off = rng.choice((rng.randrange(total + 1), rng.randrange(total + 1), total + rng.randrange(4)))
        out.append((off, rng.choice((0, 1, rng.randrange(total // 2 + 2), total, U64 - off, U64))))
    return out


def well_formed(e, level=9):
    """decode_index_check's rules, restated"""
    run = 0
    for k in range(e.size):
        assert int(e["end_bit"][k]) > int(e["bit_pos"][k]), k
        assert k == 0 or int(e["bit_pos"][k]) > int(e["bit_pos"][k - 1]), k
        assert int(e["out_off"][k]) == run, k
        assert 1 <= int(e["level"][k]) <= level, k
        run += int(e["out_len"][k])
    return run


@pytest.mark.parametrize("with_points", [False, True])
def test_subindex_reads_the_same_bytes(native, with_points):
    import banzai_amd
    rng = random.Random(31 + with_points)
    for case in range(150):
        index = synthetic(rng, rng.randrange(0, 14), with_points)
        e, total = index.entries, index.size
        truth = rng.randbytes(total)
        ranges = random_ranges(rng, total, rng.randrange(0, 65))
        sub = banzai_amd._subindex(index, ranges)
        touched = sub.touched.tolist()
        # the touched entries, byte by byte
        want = set()
        for off, n in ranges:
            for k in range(e.size):
                if n and off < int(e["out_off"][k]) + int(e["out_len"][k]) and min(off + n, total) > int(e["out_off"][k]):
                    want.add(k)
        assert touched == sorted(want), case
        # a well-formed index of exactly those blocks, everything but the positions kept
        assert well_formed(sub.entries) == sum(int(e["out_len"][k]) for k in touched)
        for field in ("out_len", "crc", "stream", "level"):
            assert sub.entries[field].tolist() == e[field][touched].tolist()
        assert (sub.entries["end_bit"] - sub.entries["bit_pos"]).tolist() == (e["end_bit"] - e["bit_pos"])[touched].tolist()
        assert banzai_amd.BlockIndex._ill_formed(sub.entries) is None
        # the runs, laid back to back, hold every touched block where its entry says: compare bit for bit through a source
        # whose every byte is its own position
        runs = sub.runs.tolist()
        for (lo, hi), (lo2, _) in zip(runs, runs[1:]):
            assert lo < hi < lo2 + 1
        where = [p for lo, hi in runs for p in range(lo, hi)]  # buffer byte -> source byte
        for j, k in enumerate(touched):
            b0, b1 = int(sub.entries["bit_pos"][j]), int(sub.entries["end_bit"][j])
            assert b0 % 8 == int(e["bit_pos"][k]) % 8 and (b1 + 7) // 8 <= len(where)
            assert where[b0 // 8:(b1 + 7) // 8] == list(range(int(e["bit_pos"][k]) // 8, (int(e["end_bit"][k]) + 7) // 8)), (case, j)
        n_runs = sum(1 for j, k in enumerate(touched) if j == 0 or touched[j - 1] != k - 1)
        assert len(runs) == n_runs
        # every translated range reads the same bytes of the touched blocks' bytes alone
        truth_sub = b"".join(truth[int(e["out_off"][k]):int(e["out_off"][k]) + int(e["out_len"][k])] for k in touched)
        assert len(sub.ranges) == len(ranges)
        for (off, n), (soff, sn) in zip(ranges, sub.ranges.tolist()):
            assert truth_sub[soff:soff + sn] == (truth[off:off + n] if off < total else b""), (case, off, n)
            assert soff + sn <= len(truth_sub)
        # the points of those entries, in order, moved with their blocks
        if with_points:
            p = index.points
            keep = [i for i in range(p.size) if int(p["entry"][i]) in want]
            assert sub.points.size == len(keep)
            assert [touched[j] for j in sub.points["entry"].tolist()] == p["entry"][keep].tolist()
            assert sub.points["group"].tolist() == p["group"][keep].tolist()
            order = list(zip(sub.points["entry"].tolist(), sub.points["group"].tolist()))
            assert order == sorted(order)
            for i, q in zip(keep, range(len(keep))):
                j = int(sub.points["entry"][q])
                assert int(sub.points["bit_pos"][q]) - int(sub.entries["bit_pos"][j]) == int(p["bit_pos"][i]) - int(e["bit_pos"][int(p["entry"][i])])
            assert banzai_amd.SyncIndex._ill_formed(sub.entries, sub.points) is None
        else:
            assert sub.points is None


def test_index_spans_binding(native):
    rng = random.Random(5)
    index = synthetic(rng, 9, False)
    e = index.entries
    touched, lo, hi, total = native.index_spans(e, [(int(e["out_off"][6]), 1), (0, 1), (int(e["out_off"][2]) - 1, 2), (index.size, 9), (3, 0)])
    assert touched.tolist() == [0, 1, 2, 6] and total == 4
    assert (lo, hi) == (int(e["bit_pos"][0]) // 8, (int(e["end_bit"][6]) + 7) // 8)
    assert native.index_spans(e, [])[0].size == 0 and native.index_spans(e, [(index.size, U64)])[1:] == (0, 0, 0)
    assert native.index_spans(e[:0], [(0, 5)]) [1:] == (0, 0, 0)
    assert native.index_spans(e, [(0, U64), (5, U64)])[3] == 2 * index.size - 5
    # too little room: BZH_E_CAP with the count set; a null pointer: BZH_E_ARG
    L = native.lib()
    r, rp = native._ranges([(0, U64)])
    ep = e.ctypes.data_as(native.idxp)
    cnt, a, b, c = ctypes.c_size_t(0), ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    room = np.zeros(3, np.uint32)
    assert L.bzh_index_spans(ep, e.size, rp, 1, native.ptr(room, native.u32p), 3, ctypes.byref(cnt), ctypes.byref(a), ctypes.byref(b),
                             ctypes.byref(c)) == -4
    assert cnt.value == 9 and c.value == index.size
    assert L.bzh_index_spans(ep, e.size, rp, 1, None, 0, ctypes.byref(cnt), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == -4
    assert L.bzh_index_spans(ep, e.size, rp, 1, None, 3, ctypes.byref(cnt), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == -1
    assert L.bzh_index_spans(ep, e.size, None, 1, native.ptr(room, native.u32p), 3, ctypes.byref(cnt), ctypes.byref(a), ctypes.byref(b),
                             ctypes.byref(c)) == -1
    assert L.bzh_index_spans(ep, e.size, rp, 1, native.ptr(room, native.u32p), 3, None, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == -1


def test_argument_errors_without_a_device(native):
    import banzai_amd
    L = native.lib()
    got = ctypes.c_size_t(7)
    assert L.bzh_decode_ranges(None, None, 0, 0, None, 0, None, 0, None, 0, None, 0, None, None, ctypes.byref(got)) == -1
    assert L.bzh_decode_ranges_device(None, None, 0, 0, None, 0, None, 0, None, 0, None, 0, None, None, ctypes.byref(got)) == -1
    assert L.bzh_get_decode_ranges_stats(None, None) == -1
    for bad in ([(1,)], [(1, 2, 3)], [5]):
        with pytest.raises((TypeError, ValueError)):
            native._ranges(bad)
    for bad in ([(-1, 2)], [(1, -2)]):
        with pytest.raises(ValueError):
            native._ranges(bad)
    for bad in ([(1.0, 2)], [("1", 2)], [(True, 2)]):
        with pytest.raises(TypeError):
            native._ranges(bad)
    assert native._ranges([(1, 2**70)])[0]["len"][0] == U64  # saturates
    index = synthetic(random.Random(1), 3, False)
    with pytest.raises(TypeError):
        banzai_amd.decompress_ranges("text", index, [(0, 1)])
    with pytest.raises(TypeError):
        banzai_amd.decompress_ranges(b"", index.entries, [(0, 1)])
    with pytest.raises(ValueError):
        banzai_amd.decompress_ranges(b"", index, [(0, -1)])
