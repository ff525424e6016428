"""GPU: every branch of the encode driver (api.hip: encode_range, run_lanes, encode_many and their callers) at level 1, on inputs
of a few blocks -- one batch gated and framed on the device, several batches on one lane, two lanes, streaming passes that start
inside a word, ranges, the index hand-off, many streams, the capacity edge and the counters.  The expected stream is the
oracle's, byte for byte; the full-size tests of the same paths are in test_gpu_parity.py, test_gpu_many.py and
test_gpu_encode_index.py."""
import functools

import numpy as np
import pytest

from tests import cases

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def data(name):
    big = cases.gen(360_000, "text", 31) + cases.gen(40_000, "longruns", 31) + cases.repeats(260_000, 31)  # 7 blocks
    return {"big": big, "two": big[:150_000], "q": b"q"}[name]


@pytest.fixture(scope="module")
def want(oracle):
    """the oracle's stream of every input, computed once"""
    return {name: oracle.encode(data(name), 1) for name in ("big", "two", "q")}


@pytest.fixture(scope="module")
def c8(native):
    c = native.Context(0, 1, 8)
    yield c
    c.close()


@pytest.fixture(scope="module")
def c2(native):
    c = native.Context(0, 1, 2)
    yield c
    c.close()


def plan_of(ctx, d):
    """the block table of `d` by the split alone (bzh_rle1_split): [(in_off, in_len, rle_len, crc)]"""
    return ctx.rle1_split(d, want_bytes=False)[0]


def device_in(d):
    import torch
    d_in = torch.zeros(len(d) + 16, dtype=torch.uint8, device="cuda:0")
    d_in[:len(d)] = torch.frombuffer(bytearray(d), dtype=torch.uint8).to("cuda:0")
    return d_in


def device_out(room, fill=0):
    import torch
    return torch.full((room,), fill, dtype=torch.uint8, device="cuda:0")


# ---- a. one batch: zeroed, checked, gated and framed on the device ---------------------------------------------------------
@pytest.mark.parametrize("name", ["two", "q"])
def test_one_batch(c8, want, name):
    assert c8.encode(data(name)) == want[name]


# ---- b. several batches, one lane: the host zeroes and checks -------------------------------------------------------------
def test_several_batches_one_lane(c2, want):
    assert -(-len(plan_of(c2, data("big"))) // 2) >= 4  # jobs of 2 blocks
    assert c2.encode(data("big")) == want["big"]


# ---- c. two lanes ------------------------------------------------------------------------------------------------------------
def test_two_lanes(native, want):
    with native.Context(0, 1, 4) as ctx:  # lanes of 2 blocks: 7 blocks in 4 jobs, each lane's arena used twice
        ctx.set_lanes(2)
        assert ctx.encode(data("big")) == want["big"]
    with native.Context(0, 1, 8) as ctx:
        ctx.set_lanes(2)
        assert ctx.encode(data("two")) == want["two"]  # one batch would do: a job for either lane all the same
        assert ctx.encode(data("q")) == want["q"]      # one job, one lane idle
        ctx.set_lanes(1)
        assert ctx.encode(data("q")) == want["q"] and ctx.encode(data("two")) == want["two"]


# ---- d. streaming: passes that start inside a word ------------------------------------------------------------------------
def stream_pieces(ctx, d, cuts):
    ctx.stream_begin(chunk_bytes=65536)
    out, pos = [], 0
    for c in cuts:
        out.append(ctx.stream_feed(d[pos:pos + c]))
        pos += c
    assert pos < len(d)
    out.append(ctx.stream_feed(d[pos:], eof=True))
    assert ctx.stream_consumed() == len(d)
    return out


@pytest.mark.parametrize("which,cuts", [("c8", [100_001, 33_333, 170_000, 7, 120_000, 99_999]),  # every pass one batch: the seed goes through pack_gate
                                        ("c2", [400_000, 250_000])])                              # passes of several batches: through the host's copy
def test_streaming_seed_word(request, want, which, cuts):
    ctx = request.getfixturevalue(which)
    pieces = stream_pieces(ctx, data("big"), cuts)
    assert b"".join(pieces) == want["big"]
    # A pass behind the first starts where a block of the stream starts, and by the oracle's stream no block but the first
    # starts on a word edge.  There was such a pass: bytes beyond the 4 of the header came out before the last feed, so a pass
    # had released blocks before the one the last feed started.
    ent, _, _ = ctx.decode_index(want["big"])
    assert len(ent) == 7 and all(int(p) % 32 != 0 for p in ent["bit_pos"][1:])
    assert sum(len(p) for p in pieces[:-1]) > 4


# ---- e. ranges --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["c2", "c8"])
def test_ranges(request, want, which):
    ctx = request.getfixturevalue(which)
    d = data("big")
    cap = (len(d) + (1 << 16)) & ~3
    d_in, d_out = device_in(d), device_out(cap)
    blocks = ctx.plan_device(d_in.data_ptr(), len(d))
    nb = len(blocks)
    assert nb == 7
    segs, keep = [], []
    for b0, b1 in ((0, 3), (3, nb)):
        buf = device_out(cap)
        segs.append((buf.data_ptr(), ctx.encode_range_device(b0, b1, buf.data_ptr(), cap)))
        keep.append(buf)
    ln = ctx.assemble_device(segs, [b[3] for b in blocks], d_out.data_ptr(), cap)
    assert d_out[:ln].cpu().numpy().tobytes() == want["big"]


# ---- f. the index hand-off --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["c8", "c2"])
def test_index(native, request, c8, want, which):
    ctx = request.getfixturevalue(which)
    stream, ent, pts = ctx.encode_index(data("big"), 16)
    assert stream == want["big"]
    went, wpts, _, used = c8.decode_index_sync(stream, 16)
    assert used == len(stream) and len(ent) == 7 and len(pts) > 7
    assert ent.tobytes() == went.tobytes() and len(pts) == len(wpts)
    for field in native.SYNC_DTYPE.names:
        assert np.array_equal(pts[field], wpts[field]), field


# ---- g. many streams --------------------------------------------------------------------------------------------------------
def test_many(c2, oracle):
    single = [cases.gen(40_000 + k, "text" if k & 1 else "random", k) for k in range(3)]
    three = data("big")[:250_000]
    assert len(plan_of(c2, three)) == 3
    items = [b"", single[0], three, b"", single[1], single[2], b""]  # batches of 2: `three` ends the first and fills the second
    for got, item in zip(c2.encode_many(items), items):
        assert got == oracle.encode(item, 1), len(item)
    assert c2.encode_many([b"", b"", b""]) == [oracle.encode(b"", 1)] * 3


# ---- h. the capacity edge of the host-mediated path ------------------------------------------------------------------------
@pytest.mark.parametrize("max_batch,lanes", [(2, 1), (4, 2)])
def test_capacity_edge(native, want, max_batch, lanes):
    """exactly the room include/bzhip.h asks for -- the stream rounded up to 4 bytes, plus 4: nothing is written behind it; 8
    bytes less: BZH_E_CAP (the footer no longer fits), and with half the room too (a batch no longer fits); the context encodes
    the same input afterwards"""
    d = data("big")
    need = (len(want["big"]) + 3) // 4 * 4 + 4
    d_in, d_out = device_in(d), device_out(need + 64, 0xA5)
    with native.Context(0, 1, max_batch) as ctx:
        ctx.set_lanes(lanes)
        for cap in (need - 8, need // 8 * 4):
            with pytest.raises(native.BzhError) as e:
                ctx.encode_device(d_in.data_ptr(), len(d), d_out.data_ptr(), cap)
            assert e.value.status == -4
        d_out.fill_(0xA5)
        ln = ctx.encode_device(d_in.data_ptr(), len(d), d_out.data_ptr(), need)
        got = d_out.cpu().numpy()
        assert got[:ln].tobytes() == want["big"] and bool((got[need:] == 0xA5).all())
        assert ctx.encode(d) == want["big"]


# ---- i. the counters of the three drivers ----------------------------------------------------------------------------------
def test_counters(native, c8, c2, want):
    d = data("big")
    plan = plan_of(c8, d)
    with native.Context(0, 1, 4) as lanes:
        lanes.set_lanes(2)
        for profiling in (False, True):
            syms = []
            for ctx in (c8, c2, lanes):  # one batch; several batches; two lanes
                ctx.set_profiling(profiling)
                try:
                    assert ctx.encode(d) == want["big"]
                    st = ctx.stats()
                finally:
                    ctx.set_profiling(False)
                assert st["raw_bytes"] == len(d) and st["blocks"] == len(plan) and st["rle_bytes"] == sum(b[2] for b in plan)
                assert (32 + st["out_bits"] + 80 + 7) // 8 == len(want["big"])
                syms.append(st["mtf_syms"])
            if profiling:
                assert syms[0] > 0 and syms[0] == syms[1] == syms[2], syms
