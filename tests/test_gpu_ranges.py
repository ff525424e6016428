"""GPU: many byte ranges in one call (bzh_decode_ranges*, banzai_amd.decompress_ranges, IndexedReader.readv) -- every touched
block decoded once, in shared batches, its tiles expanded once and copied to every piece that meets them (unrle_walk_pieces).
The truth is bz2.decompress(stream)[off:off+len] throughout.  The context takes batches of 2 blocks, so four touched blocks are
two batches and a range over blocks 1 and 2 has its pieces in both.  Damaged inputs are a short fixed list."""
import bz2
import functools
import io
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U64 = 2**64 - 1


@functools.lru_cache(maxsize=None)
def text(n, seed, words=40):
    """n bytes of words drawn from a small seeded vocabulary (tests/test_gpu_index.py's generator): few symbols keep the serial
    entropy stage, which is nearly all a read costs, short"""
    rng = random.Random(seed)
    vocab = ["".join(rng.choices("etaoinshrdlucmfwypvbgkqjxz", k=rng.randrange(2, 11))) for _ in range(words)]
    return " ".join(rng.choices(vocab, k=n // 4)).encode()[:n]


@pytest.fixture(scope="module")
def dec(native):
    c = native.Context(0, 9, 2)
    yield c
    c.close()


@pytest.fixture(scope="module")
def four(dec):
    """a level-1 stream of 350,000 bytes (4 blocks), its truth, its index and its sync points at interval 4 -- computed once,
    never changed"""
    s = bz2.compress(text(350_000, 41), 1)
    truth = bz2.decompress(s)
    ent, pts, total, used = dec.decode_index_sync(s, 4)
    assert len(ent) == 4 and total == len(truth) and used == len(s) and len(pts) > 8
    ent.setflags(write=False)
    pts.setflags(write=False)
    return s, truth, ent, pts


def clip(truth, off, n):
    return truth[off:off + n] if off < len(truth) else b""


def touched_blocks(ent, ranges):
    total = int(ent["out_off"][-1]) + int(ent["out_len"][-1])
    hit = set()
    for off, n in ranges:
        end = min(off + n, total)
        for k, e in enumerate(ent):
            if off < end and off < int(e["out_off"]) + int(e["out_len"]) and end > int(e["out_off"]):
                hit.add(k)
    return hit


def check(dec, s, ent, truth, ranges, points=None):
    """one call over `ranges`: every range's bytes, the layout, the counters"""
    blob, offs, lens = dec.decode_ranges(s, ent, ranges, points)
    want = [clip(truth, off, n) for off, n in ranges]
    run = 0
    for r, w in enumerate(want):
        assert offs[r] == run and lens[r] == len(w), (r, ranges[r])
        assert blob[run:run + len(w)] == w, (r, ranges[r])
        run += len(w)
    assert len(blob) == run
    st, ds = dec.decode_ranges_stats(), dec.decode_stats()
    hit = touched_blocks(ent, ranges)
    assert st["ranges"] == len(ranges) and st["blocks_touched"] == len(hit) == ds["blocks"] and ds["out_bytes"] == run
    assert st["batches"] == (len(hit) + 1) // 2 and ds["candidates"] == 0
    return st


# ---- 1. basic reads ----------------------------------------------------------------------------------------------------
def test_basic_reads(dec, native, four):
    s, truth, ent, _ = four
    total = len(truth)
    rng = random.Random(7)
    ranges = [(rng.randrange(total), rng.randrange(10_001)) for _ in range(200)]
    ranges += [(0, 0), (0, 1), (total - 1, 1), (0, total), (total, 5), (total + 9, 5), (total - 3, U64), (17, U64), (U64, U64)]
    for e in ent:
        b, n = int(e["out_off"]), int(e["out_len"])
        ranges += [(b, n), (b - 1, 1) if b else (0, 1), (b, 1), (b - 1, 2) if b else (0, 2), (b + n - 1, 1), (b + n - 1, 2)]
    ranges += [(1234, 567)] * 3 + [(100_000, 50_000), (110_000, 10)]
    st = check(dec, s, ent, truth, ranges)
    assert st["blocks_touched"] == 4 and st["blocks_whole"] == 0
    assert st["pieces"] == sum(len(touched_blocks(ent, [r])) for r in ranges)
    check(dec, s, ent, truth, ranges[::-1])
    check(dec, s, ent, truth, sorted(ranges, reverse=True))
    check(dec, s, ent, truth, [])
    assert native.index_spans(ent, ranges)[0].tolist() == [0, 1, 2, 3]
    assert native.index_spans(ent, ranges)[3] == sum(len(clip(truth, o, n)) for o, n in ranges)


# ---- 2. sparse touch, and the entry-list form of the segments ----------------------------------------------------------
def test_sparse_touch_with_and_without_sync_points(dec, native, four):
    s, truth, ent, pts = four
    b3 = int(ent[3]["out_off"])
    ranges = [(b3 + 100, 4096), (10, 300), (b3 + 50, 60), (int(ent[0]["out_len"]) - 1, 1)]
    for points in (None, pts):
        st = check(dec, s, ent, truth, ranges, points)
        assert st["blocks_touched"] == 2 and st["batches"] == 1
    touched, lo, hi, _ = native.index_spans(ent, ranges)
    assert touched.tolist() == [0, 3] and (lo, hi) == (int(ent[0]["bit_pos"]) // 8, (int(ent[3]["end_bit"]) + 7) // 8)
    # every block in segments, across both batches
    rng = random.Random(8)
    check(dec, s, ent, truth, [(rng.randrange(len(truth)), rng.randrange(3000)) for _ in range(50)], pts)


# ---- 3. a single range is decode_range -------------------------------------------------------------------------------
def test_single_range_and_whole_blocks(dec, four):
    s, truth, ent, _ = four
    b1, n1 = int(ent[1]["out_off"]), int(ent[1]["out_len"])
    for off, n, whole in ((b1, n1, 1), (b1 + 5, n1 - 9, 0), (b1 - 7, n1 + 20, 1), (0, len(truth), 4)):
        blob, offs, lens = dec.decode_ranges(s, ent, [(off, n)])
        assert dec.decode_ranges_stats()["blocks_whole"] == whole, (off, n)
        assert blob == dec.decode_range(s, ent, off, n) == truth[off:off + n] and offs == [0] and lens == [n]
    # a second range touching the block: no longer whole, the same bytes
    st = check(dec, s, ent, truth, [(b1, n1), (b1 + 100, 1)])
    assert st["blocks_whole"] == 0 and st["blocks_touched"] == 1 and st["pieces"] == 2
    st = check(dec, s, ent, truth, [(b1, n1), (b1 + n1, 1), (5, 0)])  # the neighbour touched instead
    assert st["blocks_whole"] == 1 and st["blocks_touched"] == 2


def test_one_range_is_one_range(dec, four):
    """decode_range[_sync] and decode_ranges of the same one range: the same bytes, the truth's, with and without sync points"""
    s, truth, ent, pts = four
    b1, n1 = int(ent[1]["out_off"]), int(ent[1]["out_len"])
    b2, n2 = int(ent[2]["out_off"]), int(ent[2]["out_len"])
    windows = [(b1, n1),                  # a whole block
               (b1 + 5, n1 - 5),          # a block cut at its head
               (b1, n1 - 5),              # a block cut at its tail
               (b1 + n1 // 2, 10),        # 10 bytes inside one block
               (0, len(truth)),           # the whole output: two batches
               (b1 + 100, n1 + n2 // 2)]  # from inside block 1 to inside block 2: a batch of two cut blocks
    assert b1 + 100 + n1 + n2 // 2 < b2 + n2
    for points in (None, pts):
        for off, n in windows:
            one = dec.decode_range(s, ent, off, n) if points is None else dec.decode_range_sync(s, ent, points, off, n)
            blob, offs, lens = dec.decode_ranges(s, ent, [(off, n)], points)
            assert one == blob == truth[off:off + n] and offs == [0] and lens == [n], (off, n, points is not None)


# ---- 4. several streams ----------------------------------------------------------------------------------------------
def test_several_streams(dec):
    a, b = text(250_000, 51), text(300_000, 52)
    s = bz2.compress(a, 1) + bz2.compress(b"", 5) + bz2.compress(b, 2)
    truth = a + b
    ent, total, _ = dec.decode_index(s)
    assert total == len(truth) and sorted(set(ent["stream"].tolist())) == [0, 2]
    seam = len(a)
    rng = random.Random(9)
    ranges = [(seam - 1, 2), (seam - 5000, 10_000), (seam, 1), (seam - 1, 1), (0, total)]
    ranges += [(rng.randrange(total), rng.randrange(8000)) for _ in range(40)]
    check(dec, s, ent, truth, ranges)


# ---- 5. tiles that expand past the staging buffer -------------------------------------------------------------------
def test_tiles_above_the_stage(dec):
    """cycling runs of 259 equal bytes: behind RLE1 each is ten bytes (four and a count of 251, four and a count of 0), so 4,096
    bytes behind the inverse BWT stand for some 106,000 of output, far more than the 8,192 the walk stages, and every tile is
    emitted piece by piece, run by run"""
    d = b"".join(bytes([97 + k % 7]) * 259 for k in range(300_000 // 259 + 1))[:300_000]
    s = bz2.compress(d, 1)
    ent, total, _ = dec.decode_index(s)
    assert total == len(d)
    rng = random.Random(10)
    ranges = [(259 * k + j, n) for k in (0, 1, 57, 400) for j in (0, 3, 4, 100, 257, 258) for n in (1, 2, 3)]  # inside and across runs
    # a run is ten bytes behind RLE1 (four and a count of 251, four and a count of 0), so bytes 4,096 and 8,192 behind the
    # inverse BWT begin at these output offsets: every position around the two tile edges
    edges = (409 * 259 + 256, 819 * 259 + 2)
    ranges += [(e - 20 + j, 5) for e in edges for j in range(40)] + [(edges[0] - 1000, edges[1] - edges[0] + 2000)]
    ranges += [(off, 40_000) for off in (0, 1, 99_999, 260_000, 299_000)]
    base = 150_000
    ranges += [(base + rng.randrange(2000), 1 + rng.randrange(700)) for _ in range(64)]  # 64 pieces in one tile
    check(dec, s, ent, d, ranges)
    check(dec, s, ent, d, [(0, total), (0, total)])


# ---- 6. many pieces in one tile of a text block ----------------------------------------------------------------------
def test_many_small_pieces_in_one_tile(dec, four):
    s, truth, ent, pts = four
    base = int(ent[1]["out_off"]) + 20_001
    ranges = [(base + 3 * k, 7) for k in range(1024)]
    assert 3 * 1024 + 7 <= 4096
    st = check(dec, s, ent, truth, ranges)
    assert st["blocks_touched"] == 1 and st["pieces"] == 1024
    check(dec, s, ent, truth, ranges, pts)


# ---- 7. no stray write ------------------------------------------------------------------------------------------------
def test_device_variant_writes_nothing_outside(dec, four):
    import torch
    s, truth, ent, _ = four
    b2 = int(ent[2]["out_off"])
    ranges = [(b2 - 3, 11), (5, 1), (int(ent[1]["out_off"]), int(ent[1]["out_len"])), (len(truth) - 2, 9), (b2 + 1, 4097)]
    want = b"".join(clip(truth, o, n) for o, n in ranges)
    t_in = torch.frombuffer(bytearray(s), dtype=torch.uint8).cuda()
    for shift in (0, 1, 3):
        t_out = torch.full((64 + shift + len(want) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        st, total, offs, lens = dec.decode_ranges_device(t_in.data_ptr(), len(s), ent, ranges, t_out.data_ptr() + 64 + shift, len(want))
        assert st == 0 and total == len(want)
        got = t_out.cpu().numpy().tobytes()
        assert got[64 + shift:64 + shift + len(want)] == want, shift
        assert got[:64 + shift] == b"\xA5" * (64 + shift) and got[64 + shift + len(want):] == b"\xA5" * 64, shift
    t_out = torch.full((len(want) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st, total, offs, lens = dec.decode_ranges_device(t_in.data_ptr(), len(s), ent, ranges, t_out.data_ptr(), len(want) - 1)
    assert st == -4 and total == len(want) and lens == [len(clip(truth, o, n)) for o, n in ranges] and offs[-1] == total - lens[-1]
    assert t_out.cpu().numpy().tobytes() == b"\xA5" * (len(want) + 64)
    assert "hold" in dec.last_error()


# ---- 8. damage ---------------------------------------------------------------------------------------------------------
def test_damage_is_a_status(dec, native, four):
    s, truth, ent, pts = four
    flip = (int(ent[2]["bit_pos"]) + int(ent[2]["end_bit"])) // 2
    damaged = bytearray(s)
    damaged[flip // 8] ^= 0x80 >> (flip % 8)
    damaged = bytes(damaged)
    b2, b3 = int(ent[2]["out_off"]), int(ent[3]["out_off"])
    ranges = [(b3 + 7, 100), (0, 50), (int(ent[1]["out_off"]) + 1, 5000), (b3, U64)]
    check(dec, damaged, ent, truth, ranges)  # damage in a block no range touches is not seen
    for points in (None, pts):
        with pytest.raises(native.BzhError) as e:
            dec.decode_ranges(damaged, ent, ranges + [(b2 + 1000, 1)], points)
        assert e.value.status == -6 and "index entry 2 " in str(e.value), str(e.value)
        check(dec, s, ent, truth, ranges + [(b2 + 1000, 1)], points)  # the context goes on
    # compressed bytes that do not cover the hull of the touched blocks
    lo, hi = native.index_spans(ent, ranges)[1:3]
    assert dec.decode_ranges(s[lo:hi], ent, ranges, in_byte_base=lo)[0] == b"".join(clip(truth, o, n) for o, n in ranges)
    for comp, base in ((s[lo:hi - 1], lo), (s[lo + 1:hi], lo + 1)):
        with pytest.raises(native.BzhError) as e:
            dec.decode_ranges(comp, ent, ranges, in_byte_base=base)
        assert e.value.status == -1 and "index entries 0..3" in str(e.value), str(e.value)
    # an ill-formed index is refused whatever the ranges
    bad = ent.copy()
    bad["out_off"][3] += 1
    with pytest.raises(native.BzhError) as e:
        dec.decode_ranges(s, bad, [(0, 1)])
    assert e.value.status == -1 and "index entry 3" in str(e.value)


# ---- 9. Python ---------------------------------------------------------------------------------------------------------
class Recording(io.BytesIO):
    """a file that records what is read of it: (position, bytes asked for)"""

    def __init__(self, data):
        super().__init__(data)
        self.reads = []

    def read(self, n=-1):
        self.reads.append((self.tell(), n))
        return super().read(n)


def test_python_surface(four):
    import banzai_amd
    s, truth, ent, pts = four
    blocks = banzai_amd.BlockIndex(ent, len(s))
    b3 = int(ent[3]["out_off"])
    sparse = [(b3 + 9, 4096), (3, 50), (len(truth) - 1, 10), (70_000, 0), (0, 1)]
    rng = random.Random(11)
    dense = sparse + [(rng.randrange(len(truth)), rng.randrange(5000)) for _ in range(30)]
    for index in (blocks, banzai_amd.SyncIndex(blocks, pts, 4)):
        for ranges in (sparse, dense):
            want = [clip(truth, o, n) for o, n in ranges]
            assert banzai_amd.decompress_ranges(s, index, ranges) == want
            assert banzai_amd.decompress_ranges(memoryview(s), index, np.array(ranges, dtype=banzai_amd._native.RANGE_DTYPE)) == want
            r = banzai_amd.IndexedReader(s, index)
            r.seek(1234)
            assert r.readv(ranges) == want and r.tell() == 1234
            f = Recording(s)
            r = banzai_amd.IndexedReader(f, index)
            r.seek(77)
            assert r.readv(ranges) == want and r.tell() == 77
            # one read per run of adjacent touched blocks, of exactly their byte span: blocks 0 and 3 alone for the sparse list
            hit = sorted(touched_blocks(ent, ranges))
            assert hit == ([0, 3] if ranges is sparse else [0, 1, 2, 3])
            runs = [[k] for k in hit[:1]]
            for k in hit[1:]:
                if k == runs[-1][-1] + 1:
                    runs[-1].append(k)
                else:
                    runs.append([k])
            spans = [(int(ent[r[0]]["bit_pos"]) // 8, (int(ent[r[-1]]["end_bit"]) + 7) // 8) for r in runs]
            assert f.reads == [(lo, hi - lo) for lo, hi in spans]
            assert r.read(5) == truth[77:82]
        assert banzai_amd.IndexedReader(s, index).readv([]) == []
