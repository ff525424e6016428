"""CPU: the model of the "fixed" Huffman mode (tests/fixed_model.py) -- its streams decode, its partition and table
count agree with hand-worked answers, and the input families the GPU tests (tests/test_gpu_fixed.py) rely on reach
the edges they are there for."""
import bz2
import random

import numpy as np
import pytest

from tests import cases
from tests import fixed_model as fm


def _trace(data, level=9):
    tr = []
    stream = fm.encode(data, level, tr)
    assert bz2.decompress(stream) == data
    return tr


@pytest.mark.parametrize("level", [1, 9])
@pytest.mark.parametrize("mode", cases.MODES)
def test_model_streams_decode(oracle, mode, level):
    for n in (0, 1, 4, 50, 257, 4097, 99_999, 100_001, 250_000):
        d = cases.gen(n, mode, 31)
        s = fm.encode(d, level)
        assert bz2.decompress(s) == d and oracle.decode(s, cap=len(d) + 64) == d, (mode, n)


def test_model_streams_decode_mixture(oracle):
    rng = random.Random(17)
    for k in range(12):
        d = cases.mixture(rng, 400_000)
        level = 1 if k % 2 else 9
        s = fm.encode(d, level)
        assert bz2.decompress(s) == d and oracle.decode(s, cap=len(d) + 64) == d, k


def test_partition_known_answers():
    """hand-worked: table t takes symbols while its sum stays below remaining // (ntab - t); middle tables with t odd
    give one symbol back if they took more than one; a target of 0 takes nothing"""
    P = fm.initial_partition
    assert P([5, 3, 2, 1], 4, 11, 2) == [(0, 1), (1, 4)]
    assert P([0, 6, 0, 0, 5, 1], 6, 12, 2) == [(0, 2), (2, 6)]  # zero-frequency symbols ride along
    assert P([4, 4, 4, 4, 1], 5, 17, 3) == [(0, 2), (2, 3), (3, 5)]  # t = 1 took one symbol: nothing to give back
    assert P([2, 2, 2, 2, 2, 1], 6, 11, 3) == [(0, 2), (2, 3), (3, 6)]  # t = 1 backs off from (2, 4)
    assert P([3] * 8 + [1], 9, 25, 4) == [(0, 2), (2, 3), (3, 6), (6, 9)]  # t = 2 (even) keeps its three
    assert P([2] * 12 + [1], 13, 25, 5) == [(0, 3), (3, 4), (4, 7), (7, 9), (9, 13)]  # t = 1 and t = 3 back off
    assert P([2] * 12 + [1], 13, 25, 6) == [(0, 2), (2, 3), (3, 5), (5, 7), (7, 10), (10, 13)]
    # fewer symbols than tables: after t = 2 one count is left, 1 // 3 == 1 // 2 == 0, so only the last table takes EOB
    r = P([10, 5, 20, 1], 4, 36, 6)
    assert r == [(0, 1), (1, 2), (2, 3), (3, 3), (3, 3), (3, 4)]
    lens = fm.initial_lengths(r, 4)
    assert lens.tolist() == [[0, 15, 15, 15], [15, 0, 15, 15], [15, 15, 0, 15], [15] * 4, [15] * 4, [15, 15, 15, 0]]
    assert P([7, 0, 0], 3, 7, 6) == [(0, 1)] + [(1, 1)] * 5  # everything in table 0, the rest start all-15


def test_table_count_edges():
    for m, want in ((1, 2), (199, 2), (200, 3), (599, 3), (600, 4), (1199, 4), (1200, 5), (2399, 5), (2400, 6),
                    (900_001, 6)):
        assert fm.num_tables(m) == want, m
    for target in (199, 200, 599, 600, 1199, 1200, 2399, 2400):
        tr = _trace(fm.with_m(fm.random_bytes, target))
        assert len(tr) == 1 and tr[0]["m"] == target and tr[0]["ntab"] == fm.num_tables(target)
        assert tr[0]["nsel"] == (target + 49) // 50


def test_m_counts_the_end_of_block_symbol(oracle):
    d = cases.gen(5000, "text", 3)
    rle, _, _ = oracle.rle_one(d, 9)
    b, _, hb = oracle.bwt(rle)
    syms, freqs, nsyms = oracle.mtf_and_rle(b, hb)
    assert int(syms[-1]) == nsyms - 1 and int(freqs[:nsyms].sum()) == len(syms) == fm.block_m(d)


def test_edge_families_reach_their_edges():
    """what the GPU tests lean on, stated here so that they cannot quietly lose it"""
    for target in (5000, 5001, 4999):  # the last segment full, single, one short
        tr = _trace(fm.with_m(fm.random_bytes, target))
        assert tr[0]["m"] == target and tr[0]["nsyms"] == 258 and tr[0]["ntab"] == 6  # the whole alphabet
    for target in (2450, 2451, 2449):  # two byte values, no run of four: 4 symbols, 6 tables, three of them empty
        tr = _trace(fm.with_m(fm.two_letters, target))
        q = tr[0]
        assert q["m"] == target and q["nsyms"] == 4 and q["ntab"] == 6
        assert [hi - lo for lo, hi in q["ranges"]] == [1, 1, 1, 0, 0, 1] and q["idle_table"]
    # m % 50 == 1: the last segment is EOB alone; the table that owns EOB from the start takes it in the first round
    q = _trace(fm.with_m(fm.two_letters, 2451))[0]
    assert q["segments"][0][5] == 1
    # cost ties and tables with no segment: low alphabets and periodic data
    for (mode, n, seed), tie, idle in ((("lowalpha", 50_000, 1), True, True), (("shortruns", 200_000, 2), True, False),
                                       (("periodic", 30_000, 4), False, True)):
        q = _trace(cases.gen(n, mode, seed))[0]
        assert q["tie"] == tie and any(0 in s for s in q["segments"]) == idle, mode
    # the deepest tables: a geometric histogram reaches the 17-bit limit
    assert max(q["max_len"] for q in _trace(fm.geometric())) == 17
    # the largest selector count: a full level-9 block of incompressible bytes
    tr = _trace(fm.random_bytes(1_000_000, 1))
    assert tr[0]["nsel"] >= 17_990 and len(tr) == 2


def test_model_is_deterministic_and_fast():
    import time
    d = fm.random_bytes(1_000_000, 2)
    t = time.perf_counter()
    a = fm.encode(d, 9)
    assert time.perf_counter() - t < 5.0  # well under a second per block on a normal core
    assert fm.encode(d, 9) == a


def test_canonical_codes():
    c = fm.canonical_codes(np.array([2, 3, 4, 1, 4]))
    # by length, then symbol: 3 -> 0, 0 -> 10, 1 -> 110, 2 -> 1110, 4 -> 1111
    assert c.tolist() == [0b10, 0b110, 0b1110, 0b0, 0b1111]
