"""The path model of the default-mode Huffman stage (tests/huff_paths_model.py) on CPU: its code lengths against the
oracle's for every case of tests/huff_cases.py and for seeded random histograms, its heap against the oracle's
build_table_from_freqs, and every case's record against the facts the case was built to reach."""
import numpy as np
import pytest

from tests import huff_cases as hc
from tests import huff_paths_model as hm


def _assert_model_is_oracle(oracle, s, ns, f, lens, rec):
    obits, on, olens = oracle.huffman_block(s, ns, f)
    assert olens.shape[0] == rec["ntab"]
    assert np.array_equal(lens, olens[:, :ns])
    assert on == rec["pack_start"] + sum(rec["tile_bits"])  # (the model's bit accounting: headers, tables, every tile)


@pytest.mark.parametrize("family", list(hc.FAMILIES))
def test_cases_reach_their_edges_and_model_equals_oracle(oracle, family):
    for name in hc.FAMILIES[family]:
        (_, s, ns, f, want), lens, rec = hc.analysed(name)
        assert s.size <= hc.M_MAX
        assert hc.unmet(rec, lens, want) == [], name
        _assert_model_is_oracle(oracle, s, ns, f, lens, rec)


def test_case_lists_are_the_issue_s():
    got = {(int(n.split("_")[1]), n.split("_")[2]) for n in hc.FAMILIES["alphabet"]}
    assert got == {(ns, k) for ns in hc.ALPHABETS for k in hc.HISTOGRAMS} and len(hc.ALPHABETS) == 27
    assert len(hc.FAMILIES["count"]) == len(hc.M_EDGES) * len(hc.M_ALPHABETS) == 51
    two = [hc.analysed(n)[2]["exps"][0] for n in hc.FAMILIES["two_tables"]]
    assert set(two) == set(range(9))  # accepted exponents 0..7 and the carry-on at 8
    three = [hc.analysed(n)[2]["exps"][0] for n in hc.FAMILIES["three_tables"]]
    assert set(three) == set(range(7))  # 0..4, the carry-on at 5 and 6


def test_deciding_halves_across_the_cases():
    """what huff_header chooses between, table by table"""
    halves = {n: hc.analysed(n)[2]["halves"] for n in hc.FAMILIES["two_tables"] + hc.FAMILIES["three_tables"]}
    assert halves["two_exp4_upper_then_lower"] == ["upper", "lower"]
    assert halves["two_both_upper"] == ["upper", "upper"]
    assert halves["two_carry_exp8"] == ["carry", "upper"]
    assert halves["three_carry_upper_lower"] == ["carry", "upper", "lower"]
    assert len(set(hc.analysed("three_different")[2]["exps"])) == 3
    assert hc.analysed("three_table1_nonzero")[2]["exps"][1] > 0


def test_heap_window_and_insert_edges_are_reached():
    """heap_extract looks at four levels a pass: sinks of 4..7 levels take a second pass, of 8 a third; heap_insert moves
    the passed ancestors in one store: a rise of more than one level"""
    sinks = {hc.analysed(n)[2]["max_sink"] for n in hc.FAMILIES["alphabet"] + hc.FAMILIES["count"]}
    assert {3, 4, 7, 8} <= sinks
    assert max(hc.analysed(n)[2]["max_rise"] for n in hc.FAMILIES["alphabet"]) >= 4
    for ns in (32, 33, 64, 65, 128, 129, 257, 258):  # a flat alphabet lets the moved element fall to the last level
        assert hc.analysed("alphabet_%d_flat" % ns)[2]["max_sink"] >= (ns - 1).bit_length() - 2, ns


def test_random_histograms_equal_oracle(oracle):
    rng = np.random.default_rng(20)
    for k in range(300):
        ns = int(rng.integers(3, 259))
        kind = k % 4
        if kind == 0:
            c = rng.integers(0, 60, ns - 1) * rng.integers(0, 2, ns - 1)
        elif kind == 1:
            c = np.minimum(1 << np.minimum(rng.permutation(ns - 1), 16), 3000)
        elif kind == 2:
            c = rng.geometric(0.2, ns - 1) - 1
        else:
            c = np.full(ns - 1, int(rng.integers(1, 9)))
        s, ns, f = hc.shuffled(c, k)
        try:
            lens, rec = hm.analyse(s, ns)
        except AssertionError as e:  # the freqs[num_syms] corner: out of scope, and the model must be the one to say so
            assert "num_syms" in str(e)
            continue
        _assert_model_is_oracle(oracle, s, ns, f, lens, rec)
        # the heap alone, on this input's histogram
        l1, _, _ = hm.build_lengths(ns, f)
        assert np.array_equal(np.array(l1, np.uint8), oracle.build_table_from_freqs(ns, f))


def test_model_refuses_a_range_that_starts_at_num_syms():
    """three tables, table 0 ending on the last symbol but one and table 1 on the last: table 2 would start at num_syms"""
    c = [1] * 255 + [5000]
    s, ns, f = hc.shuffled(c, 1)
    with pytest.raises(AssertionError, match="num_syms"):
        hm.analyse(s, ns)
