"""The statement the GPU's MTF + RLE2 stage rests on (banzai_amd/csrc/mtf.hip): an MTF position is non-zero exactly at a
run head of the last column -- a byte that differs from the byte before it; position 0: from the smallest present byte,
the front of the initial list -- so the whole layout of RLE2 (which positions emit a symbol, the zero run in front of
each, its RUNA / RUNB digits, every output offset, the trailing run, m) follows from the bytes alone.  Held here against
the oracle's mtf_and_rle, which knows nothing of run heads."""
import numpy as np
import pytest

from tests import cases

EDGE_N = [1, 2, 3, 15, 16, 17, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 70000]


def digits(z):
    """RUNA / RUNB symbols of a zero run of length z: floor(log2(z + 1)) (np.frexp is exact)"""
    return np.frexp(np.asarray(z, dtype=np.float64) + 1.0)[1].astype(np.int64) - 1


def layout(col, has_byte):
    """-> (m, offsets of the non-run symbols, every symbol below 2 in output order) from the run heads of `col` alone"""
    a = np.frombuffer(col, dtype=np.uint8)
    n = a.size
    front = int(np.nonzero(np.asarray(has_byte))[0][0])
    before = np.concatenate((np.array([front], dtype=np.uint8), a[:-1]))
    heads = np.nonzero(a != before)[0].astype(np.int64)
    prev = np.concatenate((np.array([-1], dtype=np.int64), heads[:-1]))
    z = heads - 1 - prev
    d = digits(z)
    offs = np.cumsum(d + 1) - 1
    tail = n - 1 - (int(heads[-1]) if heads.size else -1)
    dt = int(digits(tail))
    m = int((d + 1).sum()) + dt + 1
    runs = []
    for zz, dd in zip(np.concatenate((z, [tail])).tolist(), np.concatenate((d, [dt])).tolist()):
        runs += [((zz + 1) >> j) & 1 for j in range(dd)]
    return m, offs, np.array(runs, dtype=np.int64)


def check(oracle, col, hb):
    syms, freqs, nsyms = oracle.mtf_and_rle(col, hb)
    m, offs, runs = layout(col, hb)
    assert m == len(syms)
    body = syms[:-1].astype(np.int64)  # (the last symbol is EOB)
    assert int(syms[-1]) == nsyms - 1
    nonrun = np.nonzero(body >= 2)[0]
    assert nonrun.size == offs.size
    assert np.array_equal(nonrun, offs)
    assert np.array_equal(body[body < 2], runs)
    assert int(freqs[0]) == int((runs == 0).sum()) and int(freqs[1]) == int((runs == 1).sum())


@pytest.mark.parametrize("mode", cases.MODES)
def test_layout_from_run_heads_of_the_bwt(oracle, mode):
    for n in EDGE_N:
        col, _, hb = oracle.bwt(cases.gen(n, mode, 3))
        check(oracle, col, hb)


def test_layout_random_alphabets(oracle):
    rng = np.random.default_rng(8)
    for k in range(120):
        alpha = int(rng.integers(1, 257))
        n = int(rng.choice(EDGE_N + [int(rng.integers(1, 70000))]))
        letters = rng.choice(256, alpha, replace=False).astype(np.uint8)
        col, _, hb = oracle.bwt(letters[rng.integers(0, alpha, n)].tobytes())
        check(oracle, col, hb)


def test_layout_run_heavy_and_words(oracle):
    rng = np.random.default_rng(9)
    words = [bytes(rng.integers(97, 123, int(rng.integers(2, 9))).astype(np.uint8)) for _ in range(300)]
    for k in range(40):
        n = int(rng.integers(1, 70000))
        if k % 2:
            d = b" ".join(words[int(j)] for j in rng.integers(0, 300, n // 4 + 1))[:n]
        else:
            lens = rng.geometric(0.02, n // 20 + 1)
            d = b"".join(bytes([int(rng.integers(0, 5))]) * int(L) for L in lens)[:n]
        col, _, hb = oracle.bwt(d)
        check(oracle, col, hb)


def test_layout_first_byte_and_a_larger_symbol_map(oracle):
    """position 0 is a head exactly when its byte is not the smallest PRESENT byte, whatever else the map holds"""
    for n in (1, 2, 1024, 4097):
        for extra in ([], [3], [3, 200]):
            hb = np.zeros(256, dtype=np.uint8)
            hb[[7] + extra] = 1
            check(oracle, bytes([7]) * n, hb)
    hb = np.zeros(256, dtype=np.uint8)
    hb[[3, 7]] = 1
    check(oracle, bytes([3]) * 5 + bytes([7]) + bytes([3]) * 9, hb)
    check(oracle, bytes([7]) * 5 + bytes([3]), hb)
