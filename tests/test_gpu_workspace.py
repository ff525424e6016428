"""GPU: one context through every growth of its device memory (common.h: GrowBuf; batch.h: the carver, layout_batch) -- the arena
laid out for 8, 16 and 32 blocks, the first decode tables and hit list, the recorder's and the emitter's sync-point workspace,
the many-inputs workspace and stream layout growing, a streaming input buffer reallocated with bytes pending -- at level 1, where
a block is 100 kB.  After each growth the context must compute what a context that never grew computes."""
import bz2

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LEVEL, MAX_BATCH = 1, 32


def letters(n, seed):
    """n lower-case letters: no runs of four, so RLE1 leaves them alone and n bytes make ceil(n / 99,999) blocks"""
    a = np.random.default_rng(seed).integers(97, 123, n, dtype=np.uint8)
    a[3::4] = 32  # (a blank every fourth byte: no run reaches four)
    return a.tobytes()


def blocks_of(n):
    return -(-n // 99_999)


def stream(ctx, d, cuts):
    ctx.stream_begin(chunk_bytes=65536)
    out, pos = [], 0
    for c in cuts:
        out.append(ctx.stream_feed(d[pos:pos + c]))
        pos += c
    out.append(ctx.stream_feed(d[pos:], eof=True))
    assert ctx.stream_consumed() == len(d)
    return b"".join(out)


def index_sync(native, ctx, data, interval, max_ent, max_pts):
    """bzh_decode_index_sync in ONE call with room enough (the wrapper's sizing call ends in BZH_E_CAP, which leaves its text in
    last_error; here no call may fail)"""
    import ctypes
    src = np.frombuffer(data, dtype=np.uint8)
    ent, pts = np.empty(max_ent, dtype=native.INDEX_DTYPE), np.empty(max_pts, dtype=native.SYNC_DTYPE)
    cnt, npts, used, total = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_uint64(0)
    ctx.check(native.lib().bzh_decode_index_sync(ctx.handle, native.ptr(src), src.size, interval, ent.ctypes.data_as(native.idxp), max_ent,
                                                 ctypes.byref(cnt), pts.ctypes.data_as(native.syncp), max_pts, ctypes.byref(npts),
                                                 ctypes.byref(total), ctypes.byref(used)))
    return ent[:cnt.value], pts[:npts.value], int(total.value), int(used.value)


def test_one_context_through_every_growth(native):
    one, nine, seventeen = letters(60_000, 1), letters(850_000, 2), letters(1_650_000, 3)
    assert (blocks_of(len(one)), blocks_of(len(nine)), blocks_of(len(seventeen))) == (1, 9, 17)
    few = [b"", letters(3_000, 10), letters(120_000, 11), b"", letters(50, 12)]
    many = [b"" if k % 9 == 4 else letters(2_000 + 700 * k, 20 + k) for k in range(40)]
    # a streaming input buffer has 16 MiB of slack beyond its first feed: only a feed beyond that reallocates it
    fed = letters(18_000_000, 4)
    cuts = [50_000, 17_500_000]

    def fresh():
        return native.Context(0, LEVEL, MAX_BATCH)

    def same_as_fresh(got, call):
        with fresh() as f:
            want = call(f)
        assert got == want
        return got

    with fresh() as ctx:
        # 1-3. the arena laid out for 8 blocks, grown to 16, grown to 32
        for d in (one, nine, seventeen):
            s = same_as_fresh(ctx.encode(d), lambda f: f.encode(d))
            assert bz2.decompress(s) == d
        s17 = s
        # 4. the first decode: tables and hit list
        assert ctx.decode(s17) == seventeen
        # 5. the recorder's workspace
        ent, pts, total, used = index_sync(native, ctx, s17, 1, 32, 17 * 2002)  # (a point every 50 symbols at most)
        assert len(ent) == 17 and total == len(seventeen) and used == len(s17) and len(pts) > 17
        # 6. the emitter reserves the same workspace
        s9, ent9, pts9 = ctx.encode_index(nine, 4)
        with fresh() as f:
            w9, went9, wpts9 = f.encode_index(nine, 4)
        assert s9 == w9 and ent9.tobytes() == went9.tobytes() and pts9.tobytes() == wpts9.tobytes()
        assert len(ent9) == 9 and len(pts9) > 0 and bz2.decompress(s9) == nine
        # 7. a range across a block edge (and one across four), through the sync points of step 5
        for off, ln in ((99_000, 3_000), (333_333, 400_001)):
            assert ctx.decode_range_sync(s17, ent, pts, off, ln) == seventeen[off:off + ln]
        # 8. many inputs: 5, two of them empty; then 40, so that the workspace and the stream layout grow
        for items in (few, many):
            got = same_as_fresh(ctx.encode_many(items), lambda f: f.encode_many(items))
            assert [bz2.decompress(g) for g in got] == items
        # 9. streaming, three feeds, the second beyond the first buffer's slack with the first still pending
        s = same_as_fresh(stream(ctx, fed, cuts), lambda f: stream(f, fed, cuts))
        assert bz2.decompress(s) == fed
        # 10. the first input once more, in the arena of 32
        s = same_as_fresh(ctx.encode(one), lambda f: f.encode(one))
        assert bz2.decompress(s) == one
        assert ctx.last_error() == ""


def test_lanes_carve_the_shared_arena(native):
    """two lanes of 2 blocks, half of the arena each: 7 blocks in four jobs"""
    d = letters(650_000, 5)
    assert blocks_of(len(d)) == 7
    with native.Context(0, LEVEL, 4) as ctx:
        ctx.set_lanes(2)
        got = ctx.encode(d)
        assert ctx.last_error() == ""
    with native.Context(0, LEVEL, MAX_BATCH) as f:
        assert got == f.encode(d)
    assert bz2.decompress(got) == d
