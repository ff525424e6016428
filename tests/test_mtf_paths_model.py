"""The path model of MTF + RLE2 (tests/mtf_paths_model.py) on CPU: its symbols, m, histogram and num_syms against the
oracle's mtf_and_rle and against the independent Python model for every case of tests/mtf_cases.py at the case's tile
size and for seeded random columns at both, every case's record against the facts the case was built to reach, and the
model's sensitivity: eleven one-line mutants of the kind a kernel edit could make, each caught by the cases built for its
edge.

One mutant cannot change a symbol: `carry_last` of a half shorter than 1,024 bytes is read by nothing, because only the
last half of a block's last tile is short and the walk ends there; for every other half byte 15 of lane 63 IS the last
byte.  That mutant is held on the value itself (the record's carry_last against the column's byte), and the test says so
by asserting that its symbols equal the oracle's."""
import numpy as np
import pytest

from tests import mtf_cases as mc
from tests import mtf_paths_model as mm
from tests.golden import pymodel


@pytest.fixture(scope="module")
def truth(oracle):
    """the oracle's result per case, computed once"""
    memo = {}

    def get(name):
        if name not in memo:
            _, col, hb, _, _ = mc.case(name)
            memo[name] = oracle.mtf_and_rle(col, hb)
        return memo[name]
    return get


def _equal(got, want):
    s, m, f, ns = got
    ws, wf, wn = want
    return ns == wn and m == len(ws) and np.array_equal(s, ws) and np.array_equal(f, wf)


@pytest.mark.parametrize("family", list(mc.FAMILIES))
def test_cases_reach_their_edges_and_model_equals_oracle(truth, family):
    for name in mc.FAMILIES[family]:
        (_, col, hb, TL, want), got, rec = mc.analysed(name)
        assert rec["TL"] == TL and mc.unmet(rec, want) == [], name
        assert _equal(got, truth(name)), name
        assert got[1] <= len(col) + 1
        # carry_last of every half is the name of the half's last byte
        names, _ = mm.dense_names(hb)
        for t, h, clen, _, _, cl in rec["halves"]:
            assert cl == names[col[t * TL + h * mm.HALF + clen - 1]], name
        if rec["heads"]:
            assert rec["pos_min"] >= 1, name  # position 0 never comes from a run head


@pytest.mark.parametrize("family", list(mc.FAMILIES))
def test_cases_equal_the_independent_python_model(family):
    for name in mc.FAMILIES[family]:
        (_, col, hb, _, _), (s, m, f, ns), _ = mc.analysed(name)
        out, pns, pf = pymodel.mtf_and_rle(col, hb)
        assert pns == ns and len(out) == m and np.array_equal(np.array(out, np.uint16), s) and np.array_equal(np.array(pf, np.uint32), f), name


def test_case_lists_are_the_issue_s():
    assert mc.ALPHABETS == (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)
    assert set(mc.FAMILIES) == {"alphabet", "places", "chunks", "positions", "sweeps", "tiles", "layout"}
    alpha = set(mc.FAMILIES["alphabet"])
    for TL in mc.TILES:
        assert {"alphabet_%d_%s_t%d" % (N, f, TL) for N in mc.ALPHABETS for f in mc.FORMS} <= alpha
        assert {"alphabet_%d_last%s_t%d" % (N, w, TL) for N in mc.ALPHABETS if N > 1 for w in ("first", "late")} <= alpha
        assert {"chunks_H%d_t%d" % (H, TL) for H in (0, 1, 63, 64, 65, 128, 1024)} <= set(mc.FAMILIES["chunks"])
        assert {"chunks_clen_r%d_%s_t%d" % (r, h, TL) for r in range(16) for h in ("head", "nohead")} <= set(mc.FAMILIES["chunks"])
        assert {"tiles_%d_t%d" % (k, TL) for k in (1, 7, 8, 9, 15, 16, 17)} <= set(mc.FAMILIES["tiles"])
        assert {"positions_all_%d_t%d" % (r, TL) for r in (1, 2, 255)} <= set(mc.FAMILIES["positions"])
        assert {"places_all_in_word%d_t%d" % (w, TL) for w in range(4)} <= set(mc.FAMILIES["places"])
    assert len(alpha) == 2 * (22 * 3 + 21 * 2)
    assert mc.PLACE_EDGES == (63, 64, 127, 128, 191, 192, 255)
    assert {"chunks_prev_L%d_p%d" % (L, p) for L in (63, 34) for p in (0, 30, 31, 32, 33, 61) if (L, p) != (63, 63)} <= set(mc.FAMILIES["chunks"])
    assert all(mc.case(n)[3] == 4096 for n in mc.FAMILIES["sweeps"] + mc.FAMILIES["layout"])
    assert len(mc.FAMILIES["layout"]) == 2 * 13 * 3 + 9
    # what is listed and not reached says why
    for name, why in mc.UNREACHED.items():
        assert name in mc.NAMES and mc.case(name)[4]["unreached"] == why
    assert [n for n in mc.NAMES if "unreached" in mc.case(n)[4]] == [n for n in mc.NAMES if n in mc.UNREACHED]
    # every column but one fits a level-1 block, and that one needs the second round of mtf_prefix
    assert all(len(mc.case(n)[1]) <= mc.LEVEL1_M for n in mc.NAMES if n != mc.LONG)
    assert len(mc.case(mc.LONG)[1]) >= 524_289 and mc.analysed(mc.LONG)[2]["rounds"] == 2


def test_alphabet_forms():
    for TL in mc.TILES:
        for N in mc.ALPHABETS:
            hb = mc.case("alphabet_%d_scattered_t%d" % (N, TL))[2]
            assert int(hb.sum()) == N
            if 1 < N < 256:
                assert hb[0] and hb[255] and not hb.all() and (np.diff(np.nonzero(hb)[0]) > 1).any()
            if N >= 3:
                assert (mc.analysed("alphabet_%d_scattered_t%d" % (N, TL))[2]["first_tile"] < 0).any()
    seen = {k: set() for k in ("regs", "ebits")}
    for n in mc.FAMILIES["alphabet"]:
        for k in seen:
            seen[k].add(mc.analysed(n)[2][k])
    assert seen["regs"] == {1, 2, 3, 4} and seen["ebits"] == set(range(1, 9))


def test_chunk_and_tile_edges_across_the_cases():
    recs = [mc.analysed(n)[2] for n in mc.NAMES]
    for TL in mc.TILES:
        mine = [r for r in recs if r["TL"] == TL]
        assert {0, 1, 63, 64, 65, 128, 1024} <= {h[3] for r in mine for h in r["halves"]}
        assert {h[2] % 16 for r in mine for h in r["halves"]} == set(range(16))
        assert {1, 7, 8, 9, 15, 16, 17} <= {r["ntile"] for r in mine}
        assert max(r["max_one_pos_in_tile"] for r in mine) == TL  # one 16-bit counter holds a whole tile of heads
        assert any(len(r["no_head_tiles"]) >= 3 for r in mine)
    assert {(tuple(t["sweeps"]), t["first_sweep"]) for r in recs if r["TL"] == 4096 for t in r["tiles"]} >= \
        {((0,), 0), ((1,), 1), ((0, 1), 0), ((), None)}


def test_batch_lists():
    full = mc.batch_list(65)
    assert len(full) == 65
    for count in (63, 64):
        assert [c for c, _ in mc.batch_list(count)] == [c for c, _ in full[:count]]
    lens = [len(c) for c, _ in full[:63]]
    assert min(lens) == 1 and max(lens) == mc.LEVEL1_M
    alph = [int(np.asarray(h).sum()) for _, h in full]
    assert sum(a != b for a, b in zip(alph, alph[1:])) >= 48  # another alphabet from neighbour to neighbour


def test_batch_columns_at_both_tile_sizes(oracle):
    """the columns of the batch lists at the tile size their list runs with: 65 at 4,096, the first 63 at 2,048"""
    for k, (col, hb) in enumerate(mc.batch_list(65)):
        want = oracle.mtf_and_rle(col, hb)
        for TL in (4096,) + ((2048,) if k < 63 else ()):
            s, m, f, ns, _ = mm.analyse(col, hb, TL)
            assert _equal((s, m, f, ns), want), (k, TL)


def test_random_columns_equal_oracle(oracle):
    rng = np.random.default_rng(31)
    for k in range(240):
        N = int(rng.integers(1, 257))
        n = int(rng.integers(1, (3000, 9000, 20000, 20000)[k % 4]))
        present = np.sort(rng.choice(256, N, replace=False))
        col = mc.runny(rng, n, present, (1, 2, 6, 400)[k % 4]).tobytes()
        hb = mc.hb_of(present)
        want = oracle.mtf_and_rle(col, hb)
        for TL in mc.TILES:
            s, m, f, ns, _ = mm.analyse(col, hb, TL)
            assert _equal((s, m, f, ns), want), (k, TL, N, n)


# ---- sensitivity ----------------------------------------------------------------------------------------------------------
# mutant -> (family built for its edge, the cases of it that must each catch the mutant)
CATCH = {
    "regs_rounded_down": ("alphabet", ["alphabet_%d_literal_t%d" % (N, TL) for N in (63, 65, 127, 129, 191, 193, 255) for TL in mc.TILES]),
    "cnt_last_one_short": ("alphabet", ["alphabet_%d_lastfirst_t%d" % (N, TL) for N in mc.ALPHABETS if N > 1 for TL in mc.TILES]),
    "ebits_one_short": ("alphabet", ["alphabet_%d_lastfirst_t2048" % N for N in (2, 3, 5, 9, 17, 33, 65, 129)]),
    "xhi_dropped": ("chunks", ["chunks_prev_L63_p%d" % p for p in (0, 30, 31, 32, 33)]),
    "shift_folded": ("places", ["places_unseen_at_edges_t2048", "places_unseen_at_edges_t4096"]),
    "ts_word2_for_word3": ("places", ["places_all_in_word3_t2048", "places_all_in_word3_t4096"]),
    "sweep_carry_dropped": ("sweeps", ["sweeps_sweep0_only", "sweeps_both_run_across_2048"]),
    "first_from_sweep0_only": ("sweeps", ["sweeps_sweep1_only", "sweeps_head_on_2048"]),
    "prefix_skips_remainder": ("tiles", ["tiles_%d_t%d" % (k, TL) for k in (1, 7, 9, 15, 17) for TL in mc.TILES]),
    "round2_carry_reset": ("tiles", [mc.LONG]),
}


def _mutant_differs(name, mutant, want):
    _, col, hb, TL, _ = mc.case(name)
    try:
        s, m, f, ns, _ = mm.analyse(col, hb, TL, mutant=mutant)
    except (IndexError, AssertionError, ValueError):
        return True  # the mutant leaves the model's own bounds
    return not _equal((s, m, f, ns), want)


def test_every_mutant_is_listed():
    assert set(CATCH) | {"carry_last_byte15"} == set(mm.MUTANTS) and len(mm.MUTANTS) == 11


@pytest.mark.parametrize("mutant", list(CATCH))
def test_mutant_is_caught_by_the_cases_built_for_its_edge(truth, mutant):
    family, names = CATCH[mutant]
    assert names
    for name in names:
        assert name in mc.FAMILIES[family]
        assert _mutant_differs(name, mutant, truth(name)), (mutant, name)


def test_mutants_pass_where_their_edge_is_not(truth):
    """the other side of the edge: the same change is invisible on the neighbouring case, so it is the edge that catches it"""
    for mutant, names in (("regs_rounded_down", ["alphabet_%d_literal_t2048" % N for N in (64, 128, 192, 256)]),
                          ("prefix_skips_remainder", ["tiles_8_t2048", "tiles_16_t4096"]),
                          ("round2_carry_reset", ["tiles_17_t2048"]),
                          ("first_from_sweep0_only", ["sweeps_sweep0_only"]),
                          ("ts_word2_for_word3", ["alphabet_192_literal_t2048"])):
        for name in names:
            assert not _mutant_differs(name, mutant, truth(name)), (mutant, name)


def test_carry_last_mutant_is_held_on_the_value_itself(truth):
    """no symbol depends on carry_last of a short half (module docstring): the mutant's symbols are the oracle's on every
    clen case, and its carry_last is wrong at every residue but 0"""
    for TL in mc.TILES:
        for r in range(16):
            for h in ("head", "nohead"):
                name = "chunks_clen_r%d_%s_t%d" % (r, h, TL)
                _, col, hb, _, _ = mc.case(name)
                s, m, f, ns, rec = mm.analyse(col, hb, TL, mutant="carry_last_byte15")
                assert _equal((s, m, f, ns), truth(name)), name
                names, _ = mm.dense_names(hb)
                t, hf, clen, _, _, cl = rec["halves"][-1]
                assert clen % 16 == r and clen < mm.HALF
                right = names[col[t * TL + hf * mm.HALF + clen - 1]]
                assert (cl == right) == (r == 0), name
                assert all(x[5] == names[col[x[0] * TL + x[1] * mm.HALF + x[2] - 1]] for x in rec["halves"][:-1]), name
