"""MTF + RLE2 on the MI355X, where the walk emits the RLE2 symbols itself (banzai_amd/csrc/mtf.hip): symbols, m, histogram
and num_syms bit for bit the oracle's.  Through the stage seam one block runs with tiles of 2,048 bytes; whole streams of 64
blocks and more run with tiles of 4,096.  The inputs sit on the edges of the layout: no run head at all, digit-count
edges of the zero runs, runs across halves (1,024), tiles and several tiles, a head in the last position, a trailing run.
The walk's list, chunk and tile edges and hand-built columns in tiles of 4,096: tests/mtf_cases.py, tests/test_gpu_mtf_edges.py."""
import numpy as np
import pytest

from tests import cases

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 899_999]


def _hb(*byte_sets):
    hb = np.zeros(256, dtype=np.uint8)
    for s in byte_sets:
        hb[np.frombuffer(bytes(s), dtype=np.uint8)] = 1
    return hb


def _same(ctx, oracle, col, hb, what):
    gs, gf, gn = ctx.mtf(col, hb)
    os_, of, on = oracle.mtf_and_rle(col, hb)
    assert gn == on, what
    assert len(gs) == len(os_), (what, len(gs), len(os_))
    assert np.array_equal(gs, os_), (what, int(np.nonzero(gs != os_)[0][0]))
    assert np.array_equal(gf, of), what


def _literal(rng, n, alpha):
    """n bytes over `alpha` letters, no two neighbours equal: every byte a run head"""
    a = rng.integers(0, alpha, n, dtype=np.int64)
    if alpha > 1:
        for k in range(1, n):
            if a[k] == a[k - 1]:
                a[k] = (a[k] + 1) % alpha
    return a.astype(np.uint8)


def _runny(rng, n, alpha, mean):
    """n bytes over `alpha` letters in runs of geometric length"""
    lens = rng.geometric(1.0 / mean, max(n // max(mean // 2, 1), 1) + 8)
    vals = rng.integers(0, alpha, lens.size)
    return np.repeat(vals, lens)[:n].astype(np.uint8) if lens.sum() >= n else np.resize(np.repeat(vals, lens), n).astype(np.uint8)


@pytest.mark.parametrize("n", SIZES)
def test_one_byte_value(ctx9, oracle, n):
    col = bytes([7]) * n
    _same(ctx9, oracle, col, _hb([7]), "no head at all")
    _same(ctx9, oracle, col, _hb([3, 7]), "one head: position 0")
    _same(ctx9, oracle, col, _hb([3, 7, 200]), "one head, three names")


@pytest.mark.parametrize("edge", [1024, 2048, 4096])
def test_zero_runs_at_the_digit_count_edges(ctx9, oracle, edge):
    """a zero run of z = 2^k - 2, 2^k - 1, 2^k positions (the digit count steps at 2^k - 1) whose closing run head lies
    just before, on and just after a half (1,024), a tile of 2,048 and a tile of 4,096"""
    rng = np.random.default_rng(edge)
    for k in range(1, 20):
        for z in ((1 << k) - 2, (1 << k) - 1, 1 << k):
            for delta in (-1, 0, 1):
                h = edge + delta  # the head that closes the run
                while h - z - 1 < 0:
                    h += 4096
                pre = _literal(rng, h - z, 5) + 1  # its last byte opens the run (byte 0 is present and smaller: position 0 is a head)
                run = np.full(z, pre[-1], dtype=np.uint8)
                post = _literal(rng, 100, 5) + 1
                post[0] = pre[-1] % 5 + 1 if post[0] == pre[-1] else post[0]
                col = np.concatenate((pre, run, post)).tobytes()
                assert col[h] != col[h - 1] and len(set(col[h - z - 1:h])) == 1 and (h - z - 1 == 0 or col[h - z - 2] != col[h - z - 1])
                _same(ctx9, oracle, col, _hb(col, [0]), (k, z, delta))


def test_runs_over_whole_tiles_last_head_trailing_run(ctx9, oracle):
    rng = np.random.default_rng(5)
    lit = lambda n: (_literal(rng, n, 9) + 1).tobytes()
    for start in (0, 1, 1000, 2047, 2048):
        for length in (2048, 5 * 2048 + 13, 3 * 4096, 8 * 2048 - start):
            head = lit(start)
            x = bytes([200 if not head or head[-1] != 200 else 201])
            col = head + x * length + lit(3000)
            _same(ctx9, oracle, col, _hb(col), ("run over whole tiles", start, length))
            _same(ctx9, oracle, head + x * length, _hb(col), ("block ends in that run", start, length))
    for n in (2, 1024, 1025, 2048, 2049, 4096, 4097, 6000):
        body = lit(n - 1)
        _same(ctx9, oracle, body + bytes([77]), _hb(body, [77]), ("a head in the last position", n))
        _same(ctx9, oracle, body[:n // 2] + bytes([77]) * (n - n // 2), _hb(body, [77]), ("the block ends in a run", n))
        run_then_head = bytes([5]) * (n - 1) + bytes([6])
        _same(ctx9, oracle, run_then_head, _hb([5, 6]), ("one run, then a head in the last position", n))
        _same(ctx9, oracle, run_then_head, _hb([1, 5, 6]), ("the same behind a head at position 0", n))


@pytest.mark.parametrize("alpha", [2, 70, 256])
def test_sizes_and_alphabets(ctx9, oracle, alpha):
    """2 names: one key register; 70: two; 256: four.  Every byte a head, short runs, long runs."""
    rng = np.random.default_rng(alpha)
    for n in SIZES:
        for what, col in (("literal", _literal(rng, n, alpha)), ("runs of 3", _runny(rng, n, alpha, 3)),
                          ("runs of 40", _runny(rng, n, alpha, 40)), ("runs of 3000", _runny(rng, n, alpha, 3000))):
            hb = _hb(range(alpha))
            _same(ctx9, oracle, col.tobytes(), hb, (what, alpha, n))


@pytest.mark.parametrize("mode", cases.MODES)
def test_last_columns_of_real_blocks(ctx9, oracle, mode):
    for n in (4097, 300_000, 899_999):
        col, _, hb = oracle.bwt(cases.gen(n, mode, 12))
        _same(ctx9, oracle, col, hb, (mode, n))


def _families(total):
    """the families above, concatenated: text, random bytes, small alphabets, short and very long runs"""
    rng = np.random.default_rng(77)
    words = [bytes(rng.integers(97, 123, int(rng.integers(2, 9))).astype(np.uint8)) for _ in range(2000)]
    parts = []
    size = 0
    k = 0
    while size < total:
        kind = k % 6
        n = int(rng.integers(150_000, 450_000))
        if kind == 0:
            p = b" ".join(words[int(j)] for j in rng.integers(0, 2000, n // 5))
        elif kind == 1:
            p = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        elif kind == 2:
            p = _literal(rng, n, 2).tobytes()
        elif kind == 3:
            p = _runny(rng, n, 70, 3).tobytes()
        elif kind == 4:
            p = _runny(rng, n, 256, 3000).tobytes()
        else:
            p = cases.gen(n, "periodic", k) + cases.gen(n // 2, "longruns", k)
        parts.append(p)
        size += len(p)
        k += 1
    return b"".join(parts)


def test_whole_streams_of_64_blocks_and_more(native, oracle):
    """level 1: blocks of at most 99,999 bytes, so 10 MB (less after RLE1) make one batch of 64 blocks and more and the tiles are 4,096 bytes"""
    data = _families(10_000_000)
    want, blocks = oracle.encode(data, 1, want_blocks=True)
    assert len(blocks) >= 64
    with native.Context(0, 1, 0) as ctx:
        assert ctx.encode(data) == want
        # the same blocks, one batch, rotated by half a block: other tile and half edges
        cut = 50_001
        assert ctx.encode(data[cut:] + data[:cut]) == oracle.encode(data[cut:] + data[:cut], 1)


def test_one_batch_of_blocks_of_widely_different_lengths(native, oracle):
    """one stream per input in one batch: blocks of 1 byte to a full block side by side, 4,096-byte tiles"""
    rng = np.random.default_rng(3)
    data = _families(3_000_000)
    lens = [1, 2, 3, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 99_999, 70_000, 33_333]
    lens += [int(x) for x in rng.integers(1, 99_000, 70)]
    items, at = [], 0
    for n in lens:
        at = (at + 7919 * 13) % (len(data) - 100_000)
        items.append(data[at:at + n])
    items.append(bytes([9]) * 60_000)
    items.append(bytes([9, 9, 9, 8]) * 20_000)
    with native.Context(0, 1, 0) as ctx:
        streams = ctx.encode_many(items)
    assert len(streams) == len(items) >= 64
    for k, (x, s) in enumerate(zip(items, streams)):
        assert s == oracle.encode(x, 1), (k, len(x))
