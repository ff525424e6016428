"""GPU (-m gpu): the default-mode Huffman stage -- huff_init, huff_segments, the wavefront heap, huff_build's two attempt
halves and its serial carry-on tail, huff_header, the pack kernels -- driven to every table, scaling, range, segment and pack
edge by the cases of tests/huff_cases.py and held to the oracle bit for bit.

Before a case goes to the GPU the test asserts, from the record of tests/huff_paths_model.py, that it reaches the edge it
was built for.  The model shows every scaling below the accepted one to leave a code longer than 17 bits, and the lengths
accepted are the oracle's, so equal bits mean that huff_build and huff_header took the same attempt of the same half.

Reached: every alphabet edge, every symbol-count edge, two tables at exponents 0..7 and the carry-on at 8, three tables at
0..4 and the carry-on at 5 and 6, both deciders within one block, all range and segment edges, a one-bit tile, a thread
over three words.  The fullest tile the CPU search reached is 69,496 bits (4,096 x 17 - 136), 18 bits into a word.
Not reached within 900,001 symbols: two tables at exponent 9 (see tests/huff_cases.py)."""
import bz2

import numpy as np
import pytest

from tests import huff_cases as hc
from tests import huff_paths_model as hm

pytestmark = pytest.mark.gpu


def _check(oracle, ctx9, name):
    (_, s, ns, f, want), lens, rec = hc.analysed(name)
    assert hc.unmet(rec, lens, want) == [], name  # the builder still reaches its edge
    obits, on, olens = oracle.huffman_block(s, ns, f)
    assert np.array_equal(lens, olens[:, :ns]), name  # ... and the model that says so is the oracle's
    gbits, gn, glens = ctx9.huffman(s, ns, f)
    assert glens.shape[0] == olens.shape[0] == rec["ntab"], name
    assert np.array_equal(glens[:, :ns], olens[:, :ns]), (name, rec["exps"])
    assert gn == on, name
    assert gbits == obits, name


@pytest.mark.parametrize("ns", hc.ALPHABETS)
def test_alphabet_edges(oracle, ctx9, ns):
    """2 | 3 tables at 199 | 200, the 64-lane groups of the depth and code registers, every level of the heap: four
    histograms each"""
    for kind in hc.HISTOGRAMS:
        _check(oracle, ctx9, "alphabet_%d_%s" % (ns, kind))


@pytest.mark.parametrize("ns", hc.M_ALPHABETS)
def test_symbol_count_edges(oracle, ctx9, ns):
    """one symbol, the 50-symbol segment, the 4,096-symbol pack tile, huff_segments' 256 segments a workgroup"""
    for m in hc.M_EDGES:
        _check(oracle, ctx9, "count_%d_m%d" % (ns, m))


@pytest.mark.parametrize("name", hc.FAMILIES["two_tables"])
def test_scaling_two_tables(oracle, ctx9, name):
    _check(oracle, ctx9, name)


@pytest.mark.parametrize("name", hc.FAMILIES["three_tables"])
def test_scaling_three_tables(oracle, ctx9, name):
    _check(oracle, ctx9, name)


@pytest.mark.parametrize("name", hc.FAMILIES["ranges"] + hc.FAMILIES["segments"] + hc.FAMILIES["pack"])
def test_range_segment_and_pack_edges(oracle, ctx9, name):
    _check(oracle, ctx9, name)


def test_fullest_tile_bit_count():
    """what the search reached, written down: 4,096 symbols in 69,496 bits, of 69,632 possible"""
    _, lens, rec = hc.analysed("pack_fullest_tile")
    assert rec["tile_bits"][hc.FULL_TILE] == hc.FULL_TILE_BITS == 69_496 >= 4096 * 16
    assert (hm.SEAM_FRAME + rec["pack_start"] + sum(rec["tile_bits"][:hc.FULL_TILE])) % 32 == 18


def test_blocks_of_one_batch_decided_by_different_halves(oracle, ctx9):
    """huff_build and huff_header index lens2 and lfit by (half, batch size, block, table): five level-9 blocks in one batch,
    text (two tables, table 0 needs scaling 8 or 16) and uniform random bytes (three tables, scaling 1) in turn"""
    from banzai_amd import corpus
    text = corpus.enwik_synthetic_v2(4_600_000).tobytes()
    noise = corpus.xorshift_bytes(2_000_000).tobytes()
    d, at = b"", [1_800_000, 0]  # (the first two blocks of the text get by with less scaling)
    for k in range(5):
        src = (text, noise)[k % 2][at[k % 2]:at[k % 2] + 1_000_000]
        used = oracle.rle_one(src, 9)[2]
        d += src[:used]
        at[k % 2] += used
    ntabs, halves, off = [], [], 0
    while off < len(d):
        r, _, used = oracle.rle_one(d[off:off + 1_000_000], 9)
        b, _, hb = oracle.bwt(r)
        s, f, ns = oracle.mtf_and_rle(b, hb)
        _, rec = hm.analyse(s, ns)
        ntabs.append(rec["ntab"])
        halves.append(rec["halves"][0])
        off += used
    assert ntabs == [2, 3, 2, 3, 2]
    assert "upper" in halves and "lower" in halves and halves[1] == halves[3] == "lower"
    want = oracle.encode(d, 9)
    assert ctx9.encode(d) == want
    assert bz2.decompress(want) == d
    assert ctx9.encode_many([d]) == [want]
