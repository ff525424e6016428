"""GPU: the back of the decoder (decode.hip: back_sizes / back_emit) where the full decode, the index build and the range decode
share it and no other test drives it deterministically: a batch whose inverse BWT covers a candidate off the chain, and ranges,
the index and the sizing call across batches that hold only whole blocks, only cut blocks, or both."""
import bz2

import pytest

from tests import bz2_handbuilt, cases

pytestmark = pytest.mark.gpu

E_CAP = -4
BLOCK_MAGIC = 0x314159265359


def magics(s):
    """bit positions of the block magic in `s`, at any alignment"""
    v, n = int.from_bytes(s, "big"), len(s) * 8
    return [i for i in range(n - 47) if (v >> (n - 48 - i)) & ((1 << 48) - 1) == BLOCK_MAGIC]


# ---- A. an off-chain candidate inside a batch that has chain blocks behind it ------------------------------------------------
@pytest.fixture(scope="module")
def magic_inside():
    """a 54-byte level-1 stream whose payload spells the block magic: 14 bytes in use (16 symbols), two tables of sixteen 4-bit
    codes, so that the symbols 3 1 4 1 5 9 2 6 5 3 5 9 are written as the magic's nibbles -- and two of it, concatenated"""
    events = [13] * 14 + [2, ("run", 2), 3, ("run", 2), 4, 8, 1, 5, 4, 2, 4, 8] + [1, 2, 3]
    col = bz2_handbuilt.column_of_events(bytes(range(65, 79)), events)
    one = bz2_handbuilt.stream_of_column(col, 0, 1, [[4] * 16, [4] * 16], lambda g: 0)
    assert len(one.stream) == 54 and bz2.decompress(one.stream) == one.expected and len(one.expected) == 31
    assert magics(one.stream) == [32, 286]  # the block, and the candidate inside its payload
    two = one.stream + one.stream
    return two, bz2.decompress(two)


@pytest.mark.parametrize("max_batch", [8, 2])
def test_off_chain_candidate_inside_a_batch(native, magic_inside, max_batch):
    """max_batch 8: both blocks in one batch, slots 0 and 3 of it, the candidates at slots 1 and 4 off the chain -- the inverse BWT
    runs over slots 0..3, the rest over two.  max_batch 2: block and candidate fill a batch, the next starts at a footer."""
    s, truth = magic_inside
    assert len(truth) == 62
    with native.Context(0, 9, max_batch) as c:
        assert c.decode(s) == truth
        st = c.decode_stats()
        assert (st["blocks"], st["streams"], st["candidates_off_chain"]) == (2, 2, 2)
        ent, total, used = c.decode_index(s)
        assert total == 62 and used == len(s) and len(ent) == 2
        assert ent["out_off"].tolist() == [0, 31] and ent["out_len"].tolist() == [31, 31]
        assert ent["bit_pos"].tolist() == [32, 54 * 8 + 32] and ent["stream"].tolist() == [0, 1]
        assert c.decode_range(s, ent, 20, 25) == truth[20:45]  # both blocks cut
        assert c.decode_range(s, ent, 0, 62) == truth
        ent2, pts, total2, used2 = c.decode_index_sync(s, 1)
        assert total2 == 62 and used2 == len(s) and ent2.tobytes() == ent.tobytes()
        assert c.decode_range_sync(s, ent2, pts, 20, 25) == truth[20:45]
        assert c.decode_range_sync(s, ent2, pts, 0, 62) == truth


# ---- B. ranges, index and sizing across batches ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def twelve(native):
    """a level-1 stream of 12 blocks, a context that takes it in batches of 4, its index there and its sync points at interval 64
    -- computed once, never changed"""
    truth = cases.gen(1_150_000, "text", 3)
    s = bz2.compress(truth, 1)
    c = native.Context(0, 1, 4)
    ent, total, used = c.decode_index(s)
    assert len(ent) == 12 and total == len(truth) and used == len(s)  # (at least 11: three batches of 4)
    ent2, pts, _, _ = c.decode_index_sync(s, 64)
    assert ent2.tobytes() == ent.tobytes()
    ent.setflags(write=False)
    pts.setflags(write=False)
    yield c, s, truth, ent, pts
    c.close()


def windows(ent):
    """(offset, length, what the batches of 4 hold)"""
    lo = lambda k: int(ent[k]["out_off"])
    mid = lambda k: lo(k) + int(ent[k]["out_len"]) // 2
    return [(mid(1), mid(9) - mid(1), "three batches: cut + whole, whole only, cut only"),
            (mid(5) - 1000, 4321, "inside block 5: a batch with no whole block"),
            (lo(4), lo(8) - lo(4), "exactly blocks 4..7: a batch with no cut block")]


def test_ranges_across_batches(twelve):
    c, s, truth, ent, pts = twelve
    for off, n, what in windows(ent):
        assert 0 < n and off + n <= len(truth)
        assert c.decode_range(s, ent, off, n) == truth[off:off + n], what
        assert c.decode_range_sync(s, ent, pts, off, n) == truth[off:off + n], what + " (sync points)"


def test_index_does_not_depend_on_the_batch(native, twelve):
    c, s, truth, ent, pts = twelve
    with native.Context(0, 1, 8) as c8:
        ent8, total8, used8 = c8.decode_index(s)
    assert ent8.tobytes() == ent.tobytes() and total8 == len(truth) and used8 == len(s)


def test_sizing_across_batches(twelve):
    """cap 0: over capacity from the first batch.  cap len - 1: only the last batch trips it, the earlier ones were expanded."""
    c, s, truth, ent, pts = twelve
    for cap in (0, len(truth) - 1):
        st, out, need, used = c.decode_raw(s, cap)
        assert st == E_CAP and out is None and need == len(truth), cap
    assert c.decode(s) == truth


def test_device_range_writes_nothing_outside(twelve):
    import torch
    c, s, truth, ent, pts = twelve
    off, n, _ = windows(ent)[0]
    want = truth[off:off + n]
    t_in = torch.frombuffer(bytearray(s), dtype=torch.uint8).cuda()
    for shift in (0, 3):
        t_out = torch.full((64 + shift + n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        got = c.decode_range_device(t_in.data_ptr(), len(s), ent, off, n, t_out.data_ptr() + 64 + shift, n)
        h = t_out.cpu().numpy()
        assert got == n and h[64 + shift:64 + shift + n].tobytes() == want, shift
        assert (h[:64 + shift] == 0xA5).all() and (h[64 + shift + n:] == 0xA5).all(), shift
