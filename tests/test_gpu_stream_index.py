"""GPU: the streaming encoder records its index (bzh_stream_begin_index / _index_pending / _index_take).  The oracle throughout is
existing code: bzh_decode_index[_sync] of the produced stream and bzh_encode_index of the whole input, compared as bytes; the
stream itself against bzh_encode.  Level 1 and 350,000 bytes of text (4 blocks) unless stated otherwise."""
import functools
import io
import random

import numpy as np
import pytest

from tests import esync_model

pytestmark = pytest.mark.gpu

text = esync_model.text
K64, K256 = 64 << 10, 256 << 10


@pytest.fixture(scope="module")
def dec(native):
    c = native.Context(0, 9, 8)
    yield c
    c.close()


@pytest.fixture(scope="module")
def enc1(native):
    c = native.Context(0, 1, 8)
    yield c
    c.close()


@pytest.fixture(scope="module")
def enc1_fixed(native):
    c = native.Context(0, 1, 8)
    c.set_mode(True)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def input_of(name):
    return {
        "four": lambda: text(350_000, 41),
        "empty": lambda: b"",
        "one_byte": lambda: b"q",
        "long_run": lambda: b"\0" * 3_000_000 + text(260_000, 43),  # the run lies inside the first block: its tail is carried
    }[name]()


_truth = {}


def truth(enc, dec, name, interval, fixed=False):
    """(stream, entries bytes, points bytes) by bzh_encode / bzh_encode_index of the whole input, the index held against
    bzh_decode_index[_sync] of that stream -- computed once per (input, interval, mode), never changed"""
    key = (name, interval, fixed)
    if key not in _truth:
        data = input_of(name)
        plain = enc.encode(data)
        stream, ent, pts = enc.encode_index(data, interval)
        assert stream == plain
        if interval:
            want, wpts, _, used = dec.decode_index_sync(plain, interval)
        else:
            (want, _, used), wpts = dec.decode_index(plain), pts[:0]
        assert used == len(plain)
        assert ent.tobytes() == want.tobytes() and pts.tobytes() == wpts.tobytes()
        _truth[key] = (plain, ent.tobytes(), pts.tobytes())
    return _truth[key]


def feeds_of(data, how):
    """[(piece, eof)]"""
    if how == "one":
        return [(data, True)]
    if how == "k64":
        cuts = list(range(0, len(data), K64)) or [0]
        return [(data[c:c + K64], c == cuts[-1]) for c in cuts]
    if how == "k256":
        cuts = list(range(0, len(data), K256)) or [0]
        return [(data[c:c + K256], c == cuts[-1]) for c in cuts]
    if how == "irregular":
        rng, out, pos = random.Random(len(data) + 5), [], 0
        while pos < len(data):
            k = rng.randrange(1, 50_001)
            out.append((data[pos:pos + k], pos + k >= len(data)))
            pos += k
        return out or [(b"", True)]
    if how == "empty_last":
        return [(data[c:c + 100_003], False) for c in range(0, len(data), 100_003)] + [(b"", True)]
    raise KeyError(how)


def run_stream(native, ctx, data, how, interval, chunk, take):
    """-> (stream, entries, points, entries per take): `take` "every": after every feed; "end": once, behind the eof feed"""
    ctx.stream_begin_index(interval, chunk)
    out, ents, pts = [], [np.zeros(0, native.INDEX_DTYPE)], [np.zeros(0, native.SYNC_DTYPE)]
    for piece, eof in feeds_of(data, how):
        out.append(ctx.stream_feed(piece, eof))
        if take == "every" or eof:
            e, p = ctx.stream_index_take()
            ents.append(e)
            pts.append(p)
    assert ctx.stream_index_pending() == (0, 0)
    assert ctx.stream_consumed() == len(data)
    return b"".join(out), np.concatenate(ents), np.concatenate(pts), [len(e) for e in ents]


def check(native, enc, dec, name, how, interval, chunk, take, fixed=False):
    plain, want_e, want_p = truth(enc, dec, name, interval, fixed)
    stream, ent, pts, per_take = run_stream(native, enc, input_of(name), how, interval, chunk, take)
    assert stream == plain, (name, how, interval, chunk, take)
    assert ent.tobytes() == want_e, (name, how, interval, chunk, take, len(ent))
    assert pts.tobytes() == want_p, (name, how, interval, chunk, take, len(pts))
    return ent, pts, per_take


# ---- 1. chunkings x pass sizes x take schedules -------------------------------------------------------------------------------
@pytest.mark.parametrize("take", ["every", "end"])
@pytest.mark.parametrize("chunk", [K64, K256])
@pytest.mark.parametrize("how", ["one", "k64", "irregular", "empty_last"])
def test_chunkings(native, enc1, dec, how, chunk, take):
    """a trigger of 64 KiB makes passes that complete no block (a level-1 block takes about 100,000 bytes); 256 KiB makes
    passes of two blocks and a tail"""
    ent, pts, per_take = check(native, enc1, dec, "four", how, 16, chunk, take)
    assert len(ent) == 4 and len(pts) > 40
    if take == "every" and how == "k64" and chunk == K64:
        assert per_take.count(0) >= 2 and sum(1 for k in per_take if k) >= 3  # passes without a final block; blocks from several passes


# ---- 2. intervals, both Huffman modes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("interval", [0, 1, 16, 256])
@pytest.mark.parametrize("fixed", [False, True])
def test_intervals_and_modes(native, enc1, enc1_fixed, dec, interval, fixed):
    enc = enc1_fixed if fixed else enc1
    ent, pts, _ = check(native, enc, dec, "four", "irregular", interval, K64, "every", fixed)
    assert len(ent) == 4 and (len(pts) == 0) == (interval == 0)
    check(native, enc, dec, "four", "one", interval, K256, "end", fixed)


# ---- 3. a pass of more than one batch -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("how,chunk", [("one", K256), ("k256", K256), ("irregular", K64)])
def test_max_batch_2(native, enc1, dec, how, chunk):
    """max_batch = 2: the eof pass of the one-feed stream holds four blocks in two batches, the second one's positions
    continuing the first's inside the pass"""
    plain, want_e, want_p = truth(enc1, dec, "four", 16)
    with native.Context(0, 1, 2) as enc:
        stream, ent, pts, _ = run_stream(native, enc, input_of("four"), how, 16, chunk, "every")
    assert stream == plain and ent.tobytes() == want_e and pts.tobytes() == want_p


# ---- 4. edge inputs -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,how,chunk", [("empty", "one", K64), ("one_byte", "one", K64), ("one_byte", "empty_last", K64),
                                            ("long_run", "k256", K256), ("long_run", "irregular", K256)])
def test_edge_inputs(native, enc1, dec, name, how, chunk):
    ent, pts, per_take = check(native, enc1, dec, name, how, 16, chunk, "every")
    if name == "empty":
        assert len(ent) == 0 and len(pts) == 0 and len(truth(enc1, dec, name, 16)[0]) == 14
    if name == "one_byte":
        assert len(ent) == 1 and len(pts) == 0 and int(ent[0]["out_len"]) == 1
    if name == "long_run":
        assert int(ent[0]["out_len"]) > 3_000_000  # the first block: the whole run and text behind it
        assert per_take.count(0) >= 10             # passes that carried its tail on


# ---- 5. the take's room, the stream without index, the context afterwards -------------------------------------------------------
def test_take_with_arrays_one_too_small(native, enc1, dec):
    _, want_e, want_p = truth(enc1, dec, "four", 16)
    enc1.stream_begin_index(16, K256)
    enc1.stream_feed(input_of("four"), True)
    ne, npt = enc1.stream_index_pending()
    assert ne == 4 and npt * native.SYNC_DTYPE.itemsize == len(want_p)
    for me, mp in ((ne - 1, npt), (ne, npt - 1), (0, 0)):
        st, _, _, cnt, got = enc1.stream_index_take_raw(me, mp)
        assert (st, cnt, got) == (-4, ne, npt), (me, mp)
        assert enc1.stream_index_pending() == (ne, npt)  # nothing removed
    st, ent, pts, cnt, got = enc1.stream_index_take_raw(ne, npt)
    assert st == 0 and ent.tobytes() == want_e and pts.tobytes() == want_p
    assert enc1.stream_index_take_raw(0, 0)[0] == 0 and enc1.stream_index_pending() == (0, 0)


def test_take_on_a_stream_without_index(native, enc1, dec):
    plain = truth(enc1, dec, "four", 16)[0]
    enc1.stream_begin(K256)
    got = enc1.stream_feed(input_of("four"), True)
    assert got == plain
    assert enc1.stream_index_pending() == (0, 0)
    assert enc1.stream_index_take_raw(8, 8)[0] == -5
    with pytest.raises(native.BzhError) as e:
        enc1.stream_index_take()
    assert e.value.status == -5
    assert native.lib().bzh_stream_begin_index(enc1.handle, 32768) == -1


def test_a_context_after_an_indexed_stream(native, enc1, dec):
    plain = truth(enc1, dec, "four", 16)[0]
    data = input_of("four")
    run_stream(native, enc1, data, "k64", 16, K64, "end")
    enc1.stream_begin(K64)
    assert b"".join(enc1.stream_feed(p, eof) for p, eof in feeds_of(data, "k64")) == plain
    assert enc1.stream_index_pending() == (0, 0) and enc1.stream_index_take_raw(8, 8)[0] == -5
    assert enc1.encode(data) == plain
    # an indexed stream abandoned half way: the next begin drops what it had pending
    enc1.stream_begin_index(16, K64)
    for p, _ in feeds_of(data, "k64")[:4]:
        enc1.stream_feed(p, False)
    assert enc1.stream_index_pending()[0] >= 1
    enc1.stream_begin_index(0, K256)
    assert enc1.stream_index_pending() == (0, 0)
    assert enc1.stream_feed(data, True) == plain
    assert enc1.stream_index_take()[0].tobytes() == truth(enc1, dec, "four", 0)[1]


# ---- 6. use the result --------------------------------------------------------------------------------------------------------
def test_reads_through_the_streamed_index(native, enc1, dec):
    """A read decodes every segment of every block it touches, and every segment must arrive exactly at the next point: a read
    across a block boundary verifies all points of both blocks, those next to a pass boundary included.  Every block boundary
    is crossed, and 40 seeded offsets are read besides."""
    import banzai_amd
    data = input_of("four")
    stream, ent, pts, per_take = run_stream(native, enc1, data, "k64", 16, K64, "every")
    assert sum(1 for k in per_take if k) >= 3  # the index came from several passes
    index = banzai_amd.SyncIndex(banzai_amd.BlockIndex(ent, len(stream)), pts, 16)
    rng = random.Random(23)
    offs = [int(e["out_off"]) - 2048 for e in ent[1:]] + [0, len(data) - 4096, len(data) - 100]
    offs += [rng.randrange(len(data)) for _ in range(40)]
    assert len(offs) >= 32
    for off in offs:
        assert banzai_amd.decompress_range(stream, index, off, 4096) == data[off:off + 4096], off


def test_encode_indexed_stream(native, enc1):
    import banzai_amd
    data = input_of("four")

    class Chunks:  # a reader that yields 10,007 bytes at a time
        def __init__(self, d):
            self.d, self.pos = d, 0

        def read(self, n=-1):
            k = 10_007 if n < 0 else min(n, 10_007)
            out = self.d[self.pos:self.pos + k]
            self.pos += len(out)
            return out

    for interval, kind in ((256, banzai_amd.SyncIndex), (0, banzai_amd.BlockIndex)):
        want_out = io.BytesIO()
        want = banzai_amd.encode_indexed(io.BytesIO(data), want_out, 1, interval)
        for reader in (io.BytesIO(data), Chunks(data)):
            out = io.BytesIO()
            ix = banzai_amd.encode_indexed_stream(reader, out, 1, interval)
            assert isinstance(ix, kind) and out.getvalue() == want_out.getvalue()
            assert ix.consumed == len(want_out.getvalue()) and ix.to_bytes() == want.to_bytes()
    # a chunk below the input: several feeds, the same result
    out = io.BytesIO()
    ix = banzai_amd.encode_indexed_stream(io.BytesIO(data), out, 1, 256, chunk=70_001)
    assert out.getvalue() == want_out.getvalue() and ix.to_bytes() == banzai_amd.encode_indexed(io.BytesIO(data), io.BytesIO(), 1, 256).to_bytes()
