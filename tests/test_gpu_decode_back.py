"""GPU: the back of the decoder (decode.hip: back_sizes / back_emit) where the full decode, the index build and the range decode
share it and no other test drives it deterministically: a batch whose inverse BWT covers a candidate off the chain, ranges,
the index and the sizing call across batches that hold only whole blocks, only cut blocks, or both, and one block of three
tiles that takes every inverse-RLE1 kernel through each of its paths."""
import bz2
import random

import numpy as np
import pytest

from tests import bz2_handbuilt, cases
from tests.golden import pymodel

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


# ---- C. one block of three tiles under every inverse-RLE1 kernel -----------------------------------------------------------
PRE = b"pre"                       # a one-block stream in front: the block's output base is 3 mod 4
SEAMS = (211_459, 215_809)         # where tiles 1 and 2 begin in the block's own output
TILES = (211_459, 4_350, 923)      # what the tiles expand to: not staged (> 8,192), staged, staged and partial


@pytest.fixture(scope="module")
def three_tiles(native):
    """9,110 bytes behind RLE1 (n % 16 == 6): tile 0 is runs of 259 'a' and 258 'b' by turns, the count byte of the last of them
    is the first byte of tile 1 (entered in state 4), then literals, and in tile 2 a count of zero and a run of eleven.  The
    stream, the truth, a context and the index with its record table for the delimiter 'a' -- computed once, never changed"""
    rng = random.Random(27)
    lit = bytearray()
    while len(lit) < 5000:  # no two equal bytes side by side, so no run of four
        v = rng.choice(b"cdefghijklmnop \n")
        if not lit or lit[-1] != v:
            lit.append(v)
    x = b"xy" + b"".join((b"aaaa\xff", b"bbbb\xfe")[k % 2] for k in range(819)) + bytes(lit) + b"zzzz\x00" + b"qqq" + b"wwww\x07"
    block, whole = bz2_handbuilt.unrle(x)
    block = bytes(block)
    assert whole and len(x) == 9110 and len(x) % 16 == 6 and x[4096] == 0xFF and len(block) == sum(TILES) == 216_732
    assert [len(bz2_handbuilt.unrle(x[:k])[0]) for k in (4096, 8192)] == list(SEAMS)
    s = bz2.compress(PRE, 1) + bz2_handbuilt.stream_of_rle(x, 1)
    truth = PRE + block
    assert bz2.decompress(s) == truth
    c = native.Context(0, 1, 4)
    ent, pts, cum, nrec, total, used = c.decode_index_records(s, 0, ord("a"))
    assert len(ent) == 2 and total == len(truth) and used == len(s) and int(ent[1]["out_off"]) == len(PRE)
    for a in (ent, cum):
        a.setflags(write=False)
    yield c, s, truth, block, ent, cum, nrec
    c.close()


def test_three_tiles_full_decode_and_index(three_tiles):
    """unrle_walk<false> and <true>, not staged and staged, the block at an odd base; unrle_crc; unrle_count with every
    delimiter inside a run"""
    c, s, truth, block, ent, cum, nrec = three_tiles
    assert c.decode(s) == truth
    assert int(ent[1]["crc"]) == pymodel.checksum(block) and int(ent[1]["out_len"]) == len(block)
    ent0, total0, used0 = c.decode_index(s)
    assert ent0.tobytes() == ent.tobytes()
    d = truth.count(b"a")
    assert d == 410 * 259 and cum.tolist() == [0, 0, d] and nrec == d + 1


def test_three_tiles_windows_on_the_device(three_tiles):
    """unrle_walk_win: the whole block, windows of 1, 7 and 300 bytes at the five offsets around each tile seam and inside the
    run that the count byte at tile 1's start stands for, each at output shifts 0..3 between guards"""
    import torch
    c, s, truth, block, ent, cum, nrec = three_tiles
    B = len(PRE)
    wins = [(B, len(block))]
    wins += [(B + seam + d, n) for seam in SEAMS for d in (-2, -1, 0, 1, 2) for n in (1, 7, 300)]
    wins += [(B + SEAMS[0] + d, n) for d, n in ((3, 1), (100, 7), (120, 135), (254, 1), (254, 7), (0, 255))]
    t_in = torch.frombuffer(bytearray(s), dtype=torch.uint8).cuda()
    for off, n in wins:
        want = np.frombuffer(truth[off:off + n], dtype=np.uint8)
        assert want.size == n
        for shift in range(4):
            t_out = torch.full((64 + shift + n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            got = c.decode_range_device(t_in.data_ptr(), len(s), ent, off, n, t_out.data_ptr() + 64 + shift, n)
            h = t_out.cpu().numpy()
            assert got == n and (h[64 + shift:64 + shift + n] == want).all(), (off, n, shift)
            assert (h[:64 + shift] == 0xA5).all() and (h[64 + shift + n:] == 0xA5).all(), (off, n, shift)


def test_three_tiles_pieces_and_records(three_tiles):
    """unrle_walk_pieces in one call: four pieces meet tile 0 (not staged: emitted piece by piece), seven meet tile 1 (a
    wavefront a piece), two meet tile 2 (the workgroup).  unrle_select: one read whose boundary delimiters lie inside runs of tile 0"""
    c, s, truth, block, ent, cum, nrec = three_tiles
    B = len(PRE)
    ranges = [(B + 1, 5), (B + 1000, 300), (B + 200_000, 1000),
              (B + 211_450, 20), (B + 211_500, 100), (B + 211_700, 1), (B + 212_000, 700), (B + 213_000, 33), (B + 215_000, 500),
              (B + 215_805, 10), (B + 216_000, 732)]
    meet = lambda t: sum(1 for off, n in ranges if off - B < sum(TILES[:t + 1]) and off - B + n > sum(TILES[:t]))
    assert [meet(t) for t in range(3)] == [4, 7, 2] and ranges[-1][0] + ranges[-1][1] == len(truth)
    blob, offs, lens = c.decode_ranges(s, ent, ranges)
    assert blob == b"".join(truth[off:off + n] for off, n in ranges)
    assert list(lens) == [n for _, n in ranges] and list(offs) == [sum(n for _, n in ranges[:k]) for k in range(len(ranges))]
    st = c.decode_ranges_stats()
    assert st["ranges"] == len(ranges) and st["pieces"] == len(ranges) and st["blocks_touched"] == 1
    # records 100..799: they begin behind the 100th 'a' (inside the first run) and end with the 800th (inside the fourth 'a' run)
    pos = [i for i, b in enumerate(truth) if b == ord("a")]
    assert pos[99] + 1 == pos[100] and pos[799] + 1 == pos[800] and pos[800] - B < TILES[0]
    blob, offs, lens = c.decode_records(s, ent, cum, [(100, 700)], delim=ord("a"))
    assert blob == truth[pos[99] + 1:pos[799] + 1] and list(offs) == [0] and list(lens) == [len(blob)]
