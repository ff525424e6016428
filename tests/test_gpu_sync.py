"""GPU: sync points inside blocks -- bzh_decode_index_sync* records the entropy stage's state every `interval` groups, and
bzh_decode_range_sync* decodes every touched block in parallel segments (decode_header_kernel, decode_segment_kernel).  The
truth is bz2.decompress(stream)[off:off+len] throughout; the recorded points are held, field for field, to those of the host
model (tests/decode_host/sync_host.cpp), which is also where the damaged points of the last tests come from."""
import bz2
import ctypes
import functools
import io
import random

import numpy as np
import pytest

from tests import bz2_handbuilt, cases, sync_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dec(native):
    c = native.Context(0, 9, 8)
    yield c
    c.close()


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sync_model")
    return sync_model.build(tmp), tmp


@functools.lru_cache(maxsize=None)
def text(n, seed, words=40):
    rng = random.Random(seed)
    vocab = ["".join(rng.choices("etaoinshrdlucmfwypvbgkqjxz", k=rng.randrange(2, 11))) for _ in range(words)]
    return " ".join(rng.choices(vocab, k=n // 4)).encode()[:n]


@pytest.fixture(scope="module")
def four(dec):
    """a level-1 stream of 350,000 bytes (4 blocks): its truth, its index and its points at intervals 7 and 256 -- computed once,
    never changed"""
    s = bz2.compress(text(350_000, 41), 1)
    truth = bz2.decompress(s)
    ent, total, used = dec.decode_index(s)
    assert len(ent) == 4 and total == len(truth)
    pts = {}
    for interval in (7, 256):
        e2, p, t2, u2 = dec.decode_index_sync(s, interval)
        assert e2.tobytes() == ent.tobytes() and (t2, u2) == (total, used)
        p.setflags(write=False)
        pts[interval] = p
    ent.setflags(write=False)
    assert len(pts[7]) > 20 * len(pts[256]) > 0
    return s, truth, ent, pts


def concatenation():
    parts = [(text(250_000, 1), 1), (cases.gen(200_000, "shortruns", 2), 9), (b"", 5), (cases.gen(250_000, "longruns", 3), 3),
             (cases.gen(120_000, "random", 4), 1), (text(310_000, 5, words=300), 2)]
    return b"".join(bz2.compress(d, lv) for d, lv in parts), b"".join(d for d, _ in parts)


# ---- 1. the recorded points -----------------------------------------------------------------------------------------------
def test_index_sync_matches_index_and_host_model(dec, native, model, four):
    exe, tmp = model
    cat, _ = concatenation()  # more candidates than the recorder's workspace has slots at interval 1: the batch shrinks
    streams = [four[0], bz2.compress(sync_model.run_heavy(), 1), cat, bz2.compress(b"", 9)]
    for interval in (1, 7, 256):
        want, _ = sync_model.run(exe, tmp, streams, interval)
        for s, (blocks, wpts, _, _) in zip(streams, want):
            ent, total, used = dec.decode_index(s)
            ent2, pts, total2, used2 = dec.decode_index_sync(s, interval)
            assert ent2.tobytes() == ent.tobytes() and (total2, used2) == (total, used) and len(ent) == blocks
            assert pts.dtype == native.SYNC_DTYPE and len(pts) == len(wpts), interval
            for field in native.SYNC_DTYPE.names:
                assert np.array_equal(pts[field], wpts[field]), (interval, field)
            assert dec.decode_stats()["blocks"] == blocks


def test_interval_outside_its_range(dec, native):
    s = bz2.compress(b"abc" * 1000, 1)
    for interval in (0, 32768, 1 << 31):
        with pytest.raises(native.BzhError) as e:
            dec.decode_index_sync(s, interval)
        assert e.value.status == -1 and "interval" in str(e.value)
    ent, pts, total, _ = dec.decode_index_sync(s, 32767)
    assert len(ent) == 1 and len(pts) == 0 and total == 3000
    assert dec.decode_range_sync(s, ent, pts, 5, 10) == (b"abc" * 1000)[5:15]


def test_point_capacity(dec, native, four):
    s, truth, ent, pts = four
    src = np.frombuffer(s, dtype=np.uint8)
    cnt, npts, used, total = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_uint64(0)
    ebuf = np.zeros(4, dtype=native.INDEX_DTYPE)
    want = len(pts[256])
    for room in (0, want - 1):
        pbuf = np.zeros(max(room, 1), dtype=native.SYNC_DTYPE)
        st = native.lib().bzh_decode_index_sync(dec.handle, native.ptr(src), len(s), 256, ebuf.ctypes.data_as(native.idxp), 4, ctypes.byref(cnt),
                                                pbuf.ctypes.data_as(native.syncp) if room else None, room, ctypes.byref(npts),
                                                ctypes.byref(total), ctypes.byref(used))
        assert st == -4 and cnt.value == 4 and npts.value == want and total.value == len(truth)
    pbuf = np.zeros(want, dtype=native.SYNC_DTYPE)
    st = native.lib().bzh_decode_index_sync(dec.handle, native.ptr(src), len(s), 256, ebuf.ctypes.data_as(native.idxp), 4, ctypes.byref(cnt),
                                            pbuf.ctypes.data_as(native.syncp), want, ctypes.byref(npts), ctypes.byref(total), ctypes.byref(used))
    assert st == 0 and npts.value == want and pbuf.tobytes() == pts[256].tobytes() and ebuf.tobytes() == ent.tobytes()
    st = native.lib().bzh_decode_index_sync(dec.handle, native.ptr(src), len(s), 256, ebuf.ctypes.data_as(native.idxp), 3, ctypes.byref(cnt),
                                            pbuf.ctypes.data_as(native.syncp), want, ctypes.byref(npts), ctypes.byref(total), ctypes.byref(used))
    assert st == -4 and cnt.value == 4 and npts.value == want  # the entries do not fit: both counts are set all the same


# ---- 2. ranges ------------------------------------------------------------------------------------------------------------
def test_ranges_of_a_four_block_stream(dec, native, four):
    s, truth, ent, pts = four
    total = len(truth)
    pairs = [(0, total), (0, total + 9), (total, 5), (total + 5, 1), (7, 0), (total - 3, 10), (1, total - 2)]
    for k in range(1, 4):  # one byte either side of every block edge
        b = int(ent[k]["out_off"])
        pairs += [(b - 1, 1), (b - 1, 2), (b, 1), (b + 1, 1), (b - 1, 3), (b - 4097, 8195)]
    b1, l1 = int(ent[1]["out_off"]), int(ent[1]["out_len"])
    pairs += [(b1 + l1 // 2, 1), (b1 + l1 // 2, 100), (b1 + 10, 4096), (b1 + l1 - 200, 150)]  # inside one segment of block 1
    for interval in (7, 256):
        for off, n in pairs:
            got = dec.decode_range_sync(s, ent, pts[interval], off, n)
            assert got == truth[off:off + n], (interval, off, n)
            first, last, _, _ = native.index_span(ent, off, n)
            st = dec.decode_stats()
            assert st["blocks"] == last - first and st["candidates"] == 0 and st["out_bytes"] == len(got), (off, n)
    for off, n in pairs[:12]:
        assert dec.decode_range(s, ent, off, n) == truth[off:off + n]  # the yardstick itself
    assert dec.decode_range_sync(s, ent, pts[256][:0], b1 + 3, 5000) == dec.decode_range(s, ent, b1 + 3, 5000)  # npts = 0
    only1 = pts[256][pts[256]["entry"] == 1]  # points for one block only: the others decode as one segment each
    assert dec.decode_range_sync(s, ent, only1, 0, total) == truth


def test_python_surface(dec, four):
    import banzai_amd
    s, truth, ent, pts = four
    ix = banzai_amd.build_sync_index(s, 256)
    assert ix.points.tobytes() == pts[256].tobytes() and ix.blocks.entries.tobytes() == ent.tobytes() and ix.interval == 256
    assert ix.blocks.to_bytes() == banzai_amd.build_index(s).to_bytes()
    ix = banzai_amd.SyncIndex.from_bytes(ix.to_bytes())
    b2 = int(ent[2]["out_off"])
    for off, n in ((0, 10 ** 9), (b2 - 1, 2), (b2 + 5000, 4096), (len(truth) - 5, 50), (len(truth), 4), (3, 0)):
        assert banzai_amd.decompress_range(s, ix, off, n) == truth[off:off + n] == banzai_amd.decompress_range(s, ix.blocks, off, n)
    r, ref = banzai_amd.IndexedReader(io.BytesIO(s), ix), io.BytesIO(truth)
    for step in (("read", 10), ("seek", b2 - 3, 0), ("read", 6), ("seek", -100, 2), ("read", 500), ("seek", 150_000, 0), ("read", 120_000),
                 ("seek", 5, 0), ("read", -1)):
        if step[0] == "seek":
            assert r.seek(step[1], step[2]) == ref.seek(step[1], step[2])
        else:
            assert r.read(step[1]) == ref.read(step[1]), step
    assert banzai_amd.IndexedReader(s, ix).read() == truth
    assert banzai_amd.build_sync_index(s).interval == 256 and banzai_amd.build_sync_index(s, 7).points.tobytes() == pts[7].tobytes()


def whole_and_seams(dec, s, interval, expect_blocks=None):
    truth = bz2.decompress(s)
    ent, pts, total, _ = dec.decode_index_sync(s, interval)
    assert total == len(truth) and (expect_blocks is None or len(ent) == expect_blocks)
    assert dec.decode_range_sync(s, ent, pts, 0, total) == truth
    for k in range(1, len(ent)):
        b = int(ent[k]["out_off"])
        assert dec.decode_range_sync(s, ent, pts, b - 3, 7) == truth[b - 3:b + 4]
    return ent, pts, truth


def test_own_encoder_in_both_huffman_modes(dec, ctx1):
    d = text(230_000, 42, words=3000)
    for fixed in (False, True):
        ctx1.set_mode(fixed)
        try:
            s = ctx1.encode(d)
        finally:
            ctx1.set_mode(False)
        ent, pts, truth = whole_and_seams(dec, s, 7, expect_blocks=3)
        assert truth == d and len(pts) > 100


def test_concatenation_of_levels(dec):
    s, d = concatenation()
    ent, pts, truth = whole_and_seams(dec, s, 64)
    assert truth == d and len(set(ent["level"].tolist())) == 4 and len(pts) > 50


def test_hand_built_full_block(dec):
    full = bz2_handbuilt.stream_of_rle((b"aaaa\xff" + b"bbbb\xfe") * 10000, 1)  # nblock = 100,000: one more than encoders fill
    want = (b"a" * 259 + b"b" * 258) * 10000
    ent, pts, total, _ = dec.decode_index_sync(full, 1)
    assert len(ent) == 1 and total == len(want) and len(pts) < 8  # long runs: a handful of groups, the last segment's room is the block
    assert int(pts["out_pos"].max(initial=0)) <= 100_000
    assert dec.decode_range_sync(full, ent, pts, 0, total) == want
    assert dec.decode_range_sync(full, ent, pts, 2_585_000 - 300, 600) == want[2_585_000 - 300:2_585_000 + 300]


def test_run_heavy_at_interval_one(dec):
    d = sync_model.run_heavy()
    s = bz2.compress(d, 1)
    ent, pts, truth = whole_and_seams(dec, s, 1, expect_blocks=1)
    assert truth == d and np.any(pts["run_weight"] > 1)  # some segment starts inside a run
    for off, n in ((0, 1), (len(d) - 1, 1), (len(d) // 2, 3000)):
        assert dec.decode_range_sync(s, ent, pts, off, n) == d[off:off + n]


def test_one_level9_block(dec):
    d = text(880_000, 43, words=3000)
    s = bz2.compress(d, 9)
    ent, pts, truth = whole_and_seams(dec, s, 256, expect_blocks=1)
    assert truth == d and len(pts) >= 20
    for off, n in ((0, 4096), (len(d) - 4096, 4096), (440_000, 1 << 20)):
        assert dec.decode_range_sync(s, ent, pts, off, n) == d[off:off + n]


def test_span_only_buffer(dec, native, four):
    s, truth, ent, pts = four
    b2, b3 = int(ent[2]["out_off"]), int(ent[3]["out_off"])
    for off, n in ((b2 + 10, 50), (b2 - 1, 2), (b2 - 5, b3 - b2 + 10), (len(truth) - 3, 3)):
        first, last, lo, hi = native.index_span(ent, off, n)
        want = truth[off:off + n]
        assert dec.decode_range_sync(s[lo:hi], ent, pts[256], off, n, in_byte_base=lo) == want
        assert dec.decode_range_sync(s[lo:], ent, pts[7], off, n, in_byte_base=lo) == want
        with pytest.raises(native.BzhError) as e:
            dec.decode_range_sync(s[lo:hi - 1], ent, pts[256], off, n, in_byte_base=lo)
        assert e.value.status == -1 and f"{first}..{last - 1}" in str(e.value)
        assert dec.decode_range_sync(s[lo:hi], ent, pts[256], off, n, in_byte_base=lo) == want  # the context goes on


def test_device_variant_writes_nothing_outside(dec, four):
    import torch
    s, truth, ent, pts = four
    t_in = torch.frombuffer(bytearray(s), dtype=torch.uint8).cuda()
    b1, l1 = int(ent[1]["out_off"]), int(ent[1]["out_len"])
    windows = [(b1, 1), (b1, 4097), (b1 + l1 // 2 - 3, 9001), (b1 + l1 - 1, 1), (b1, l1), (b1 - 1, l1 + 2), (b1 - 3, 6), (0, len(truth)),
               (3, len(truth) - 6)]
    for off, n in windows:
        want = truth[off:off + n]
        for shift in (0, 1, 3):
            t_out = torch.full((64 + shift + len(want) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            got = dec.decode_range_sync_device(t_in.data_ptr(), len(s), ent, pts[256], off, n, t_out.data_ptr() + 64 + shift, len(want))
            h = t_out.cpu().numpy()
            assert got == len(want) and h[64 + shift:64 + shift + got].tobytes() == want, (off, n, shift)
            assert (h[:64 + shift] == 0xA5).all() and (h[64 + shift + got:] == 0xA5).all(), (off, n, shift)


# ---- 3. points are untrusted: a status, never a fault (after everything valid) ---------------------------------------------
def test_ill_formed_points_are_refused(dec, native, four):
    s, truth, ent, pts = four
    good = pts[256]
    second = int(np.flatnonzero(good["entry"] == 1)[0])
    rules = [("order", "group", second + 1, int(good["group"][second])),           # (entry, group) not ascending
             ("order", "entry", second, 0),
             ("entry", "entry", len(good) - 1, 4),                               # outside the index
             ("bit_pos", "bit_pos", 0, int(ent[0]["bit_pos"])),                  # not strictly inside its entry
             ("bit_pos", "bit_pos", 0, int(ent[0]["end_bit"])),
             ("bit_pos", "bit_pos", 1, int(good["bit_pos"][0])),                 # not ascending
             ("out_pos", "out_pos", 1, int(good["out_pos"][0]) - 1),             # descends
             ("out_pos", "out_pos", second - 1, 100_001),                        # beyond the level's block size
             ("run_weight", "run_weight", 0, 3), ("run_weight", "run_weight", 0, 1 << 23), ("run_weight", "run_weight", 0, 0),
             ("run", "run", 0, 1),                                               # a run with no digit pending
             ("reserved", "reserved", 2, 1), ("group", "group", 0, 0)]
    for rule, field, k, value in rules:
        bad = good.copy()
        if field == "run":
            bad["run_weight"][k] = 1
        bad[field][k] = value
        with pytest.raises(native.BzhError) as e:
            dec.decode_range_sync(s, ent, bad, 0, 10)  # (whatever the range: the points are checked as a whole)
        assert e.value.status == -1 and f"sync point {k}:" in str(e.value), (rule, field, str(e.value))
    assert dec.decode_range_sync(s, ent, good, 3, 10) == truth[3:13]


def test_wrong_points_are_a_status(dec, native, model):
    """well-formed points that are wrong for the bytes -- single-bit flips the host model found to pass the rule for ill-formed
    points and to be caught by a segment -- are BZH_E_DATA naming the entry and the point; the context goes on"""
    exe, tmp = model
    s = bz2.compress(text(120_000, 44), 1)
    truth = bz2.decompress(s)
    res, _ = sync_model.run(exe, tmp, [s], 16)
    blocks, wpts, flips, _ = res[0]
    ent, pts, total, _ = dec.decode_index_sync(s, 16)
    assert pts.tobytes() == wpts.tobytes() and blocks == len(ent) == 2
    by_field = {}
    for point, byte, bit in flips:  # one flip for every field and point the model reached, a dozen or so in all
        field = "mtf" if byte >= 32 else ("bit_pos" if byte < 8 else ("entry", "group", "out_pos", "run", "run_weight", "reserved")[(byte - 8) // 4])
        by_field.setdefault((field, point), (point, byte, bit))
    chosen = sorted(by_field.values())
    chosen = chosen[::max(1, len(chosen) // 12)][:14]
    assert len(chosen) >= 10 and len({c[0] for c in chosen}) >= 3
    for point, byte, bit in chosen:
        bad = pts.copy()
        bad.view(np.uint8).reshape(len(pts), 288)[point, byte] ^= 1 << bit
        entry = int(pts["entry"][point])
        with pytest.raises(native.BzhError) as e:
            dec.decode_range_sync(s, ent, bad, 0, total)
        assert e.value.status == -6 and f"index entry {entry} " in str(e.value) and f"sync point {point}:" in str(e.value), (point, byte, bit, str(e.value))
        assert dec.decode_range_sync(s, ent, pts, 5, 20) == truth[5:25]  # the context goes on
    # the points of another stream of the same shape: well formed or not, never bytes that are not the truth
    other = bz2.compress(text(120_000, 45), 1)
    _, opts, _, _ = dec.decode_index_sync(other, 16)
    with pytest.raises(native.BzhError) as e:
        dec.decode_range_sync(s, ent, opts, 0, total)
    assert e.value.status in (-1, -6)
    assert dec.decode_range_sync(s, ent, pts, 0, total) == truth


def test_wrong_point_behind_the_first_batch(native, model):
    """the same flips in the blocks of a second batch (4 blocks, 2 a batch): the message names the point by its number in the
    caller's array, not by its number among the batch's points"""
    exe, tmp = model
    s = bz2.compress(text(350_000, 41), 1)
    truth = bz2.decompress(s)
    res, _ = sync_model.run(exe, tmp, [s], 16)
    blocks, wpts, flips, _ = res[0]
    with native.Context(0, 1, 2) as c2:
        ent, pts, total, _ = c2.decode_index_sync(s, 16)
        assert pts.tobytes() == wpts.tobytes() and blocks == len(ent) == 4
        by_field = {}
        for point, byte, bit in flips:  # one flip for every field and point of entries 2 and 3 the model reached
            if int(pts["entry"][point]) < 2:
                continue
            field = "mtf" if byte >= 32 else ("bit_pos" if byte < 8 else ("entry", "group", "out_pos", "run", "run_weight", "reserved")[(byte - 8) // 4])
            by_field.setdefault((field, point), (point, byte, bit))
        chosen = sorted(by_field.values())
        chosen = chosen[::max(1, len(chosen) // 6)][:8]
        assert len(chosen) >= 4 and {int(pts["entry"][c[0]]) for c in chosen} == {2, 3}
        assert int(np.flatnonzero(pts["entry"] >= 2)[0]) > 0  # (the batch's first point is not the array's)
        for point, byte, bit in chosen:
            bad = pts.copy()
            bad.view(np.uint8).reshape(len(pts), 288)[point, byte] ^= 1 << bit
            entry = int(pts["entry"][point])
            with pytest.raises(native.BzhError) as e:
                c2.decode_range_sync(s, ent, bad, 0, total)
            assert e.value.status == -6 and f"index entry {entry} " in str(e.value) and f"sync point {point}:" in str(e.value), (point, byte, bit, str(e.value))
            assert c2.decode_range_sync(s, ent, pts, 5, 20) == truth[5:25]  # the context goes on
