"""The path model of the suffix sort (tests/bwt_paths_model.py) on CPU: its counts against a brute force over sorted
rotations, every edge family on both sides of its edge, and the verdicts scripts/gpu_msd_check.py relies on."""
import random

import numpy as np
import pytest

from banzai_amd import corpus
from tests import bwt_paths_model as bm
from tests import cases


def _rots(x):
    return sorted(x[i:] + x[:i] for i in range(len(x)))


def _brute_groups(x, h):
    pre = [(r * (h // len(r) + 1))[:h] for r in _rots(x)]
    return sorted(pre.count(p) for p in sorted(set(pre)))


def _brute_plan(x, tile):
    """buckets from the sorted rotations: 2-byte buckets packed (256 a unit), then level by level"""
    rots = _rots(x)

    def pre(r, k):
        return (r * (k // len(r) + 1))[:k]

    def counts(rs, k):
        out = []
        for r in rs:
            if out and out[-1][0] == pre(r, k):
                out[-1][1].append(r)
            else:
                out.append((pre(r, k), [r]))
        return out

    units = 0
    over = [0] * 6
    tiles = [0] * 6
    spans = False

    def pack(buckets, width):
        nonlocal units
        u, is_open, size, nb, pover, res = 0, False, 0, 0, False, []
        for _, rs in buckets:
            c = len(rs)
            ov = c > tile
            if not is_open or ov or pover or size + c > tile or (width and nb >= width):
                if ov:
                    res.append(rs)
                else:
                    u += 1
                is_open, size, nb = True, 0, 0
            size += c
            nb += 1
            pover = ov
        units += u
        return res

    todo = pack(counts(rots, 2), 256)
    for L in range(1, 6):
        over[L] = len(todo)
        tiles[L] = sum(-(-len(rs) // tile) for rs in todo)
        nxt = []
        for rs in todo:
            res = pack(counts(rs, L + 2), 0)
            if L == 5 and res:
                spans = True
                units += sum(-(-len(q) // tile) for q in res)
            else:
                nxt += res
        todo = nxt
    ne = len(counts(rots, 2))
    return {"units": units, "over": over, "tiles": tiles, "spans": spans, "ne": ne}


def test_groups_match_sorted_rotations():
    rng = random.Random(3)
    for _ in range(60):
        n = rng.randrange(1, 40)
        x = bytes(rng.choice(b"ab" if rng.random() < 0.5 else b"abcd") for _ in range(n))
        for h in (1, 2, 3, 5, 7, 8, 13):
            assert sorted(bm.group_sizes(x, h).tolist()) == _brute_groups(x, h), (x, h)


def test_plan_matches_sorted_rotations():
    """with a tile of a few suffixes, the split reaches every level on tiny blocks"""
    rng = random.Random(4)
    for it in range(150):
        n = rng.randrange(1, 60)
        alpha = rng.choice([b"a", b"ab", b"abc", b"abcdefgh"])
        x = bytes(rng.choice(alpha) for _ in range(n))
        tile = rng.choice([1, 2, 3, 5])
        p = bm.block_plan(x, force_new=True, tile=tile, ne_max=1 << 20)
        want = _brute_plan(x, tile)
        assert p["ne"] == want["ne"], x
        assert (p["units"], p["over"], p["tiles"], p["spans"]) == (want["units"], want["over"], want["tiles"], want["spans"]), (x, tile, p, want)


def test_units_of_256_buckets():
    """bigram_plan's unit width: the 257th bucket starts a new unit"""
    a, b = bm.fam_unit_width()
    pa, pb = bm.block_plan(a), bm.block_plan(b)
    assert (pa["ne"], pa["units"]) == (256, 1)
    assert (pb["ne"], pb["units"]) == (257, 2)


@pytest.fixture(scope="module")
def fam():
    return bm.families()


def test_families_straddle_their_edges(fam):
    P = {k: (bm.block_plan(a), bm.block_plan(b)) for k, (a, b) in fam.items() if k not in ("tail_g", "gid8", "gid7", "five_passes", "quad")}
    a, b = P["sample_n"]
    assert (len(fam["sample_n"][0]), len(fam["sample_n"][1])) == (32767, 32768)
    assert a["distinct"] is None and a["np"] and b["distinct"] * 2 < bm.MS_SAMPLES and not b["np"]
    a, b = P["sample_distinct"]
    assert (a["distinct"], b["distinct"], a["np"], b["np"]) == (2047, 2048, False, True)
    a, b = P["ne"]
    assert (a["ne"], b["ne"], a["np"], b["np"]) == (8192, 8193, True, False)
    a, b = P["over_pct"]
    n = len(fam["over_pct"][0])
    assert a["bigall"] * 100 == n * bm.MS_OVER_PCT and b["bigall"] == a["bigall"] + 1 and a["np"] and not b["np"]
    assert bm.block_plan(fam["over_pct"][1], force_new=True)["np"]
    for L in range(6):
        a, b = P[f"tile{L}"]
        assert a["np"] and b["np"], L
        if L < 5:
            assert b["over"][L + 1] == a["over"][L + 1] + 1, (L, a["over"], b["over"])
            assert b["tiles"][L + 1] == a["tiles"][L + 1] + 2, L  # (8,193 suffixes: two tiles)
        else:
            assert (a["spans"], b["spans"]) == (False, True)
    a, b = P["tile1"]
    assert (a["deeper"], b["deeper"]) == (False, True)  # levels 2-5 skipped / run
    r = [bm.round0(x, False) for x in fam["tail_g"]]
    assert (r[0]["large"], r[0]["big_records"]) == (0, 0) and r[1]["large"] > 0 and not r[1]["sweep"]
    r = [bm.round0(x, False) for x in fam["gid8"]]
    assert [x["large"] for x in r] == [4096, 4097] and [x["on_ranks"] for x in r] == [False, True]
    r = [bm.round0(x, True) for x in fam["gid7"]]
    assert [x["large"] for x in r] == [4096, 4097] and all(bm.block_plan(x)["np"] for x in fam["gid7"])
    assert [bm.round0(x, False)["large"] for x in fam["gid7"]] == [4095, 4096]  # (the other path's depth: both dense)
    r = [bm.round0(x, False) for x in fam["five_passes"]]
    assert [x["big_records"] for x in r] == [250000, 250001] and [x["passes_next"] for x in r] == [4, 5]
    assert all(len(x) > bm.FOUR_PASS_MAX for x in fam["five_passes"])
    r = [bm.round0(x, False) for x in fam["quad"]]
    assert [x["small_records"] for x in r] == [9999, 10000] and [x["big_records"] for x in r] == [0, 0]
    assert all(len(x) == 100000 for x in fam["quad"]) and [x["quad"] for x in r] == [True, False]


def test_mixed_batches_mix_paths(fam):
    for name, (lvl, mb, blocks) in bm.mixed_batches(fam).items():
        assert all(0 < len(b) <= 100000 * lvl - 1 for b in blocks), name
        for p in bm.batch_plans(blocks, lvl, mb, "default"):
            assert len(p["plans"]) >= bm.BATCH_MIN and p["msd"] and p["new"] and p["old"], name
        assert any(bm.period_shrink(b) != len(b) for b in blocks)


def test_gpu_msd_check_blocks():
    """the verdicts the blocks of scripts/gpu_msd_check.py get (its docstring): text bucket-first with oversized buckets split,
    repetitive blocks and runs kept on the 8 passes by the sample test, random bytes by their 65,536 buckets, tiny blocks
    bucket-first; the block of indented code is near-periodic and sorted as a few of its periods"""
    text = corpus.enwik_synthetic_v2(4_000_000, seed=5).tobytes()
    code = (b"    " * 3 + b"if (x[i] == y[i]) {\n" + b"        " + b"return value;\n" + b"    }\n") * 40_000

    def plan(x):
        return bm.block_plan(x[:bm.period_shrink(x)], force_new=True)
    p = plan(text[:899_999])
    assert p["np"] and p["over"][1] > 0 and p["units"] > 100
    assert plan(text[:200_000])["np"] and plan(text[:17])["np"] and plan(b"q")["np"] and plan(b"qq")["np"]
    for x in (cases.gen(899_999, "longruns", 3), cases.gen(500_000, "shortruns", 4), b"\x07" * 300_000):
        p = plan(x)
        assert not p["np"] and p["distinct"] * 2 < bm.MS_SAMPLES
    p = plan(corpus.xorshift_bytes(899_999).tobytes())
    assert not p["np"] and p["ne"] == 65536
    assert bm.period_shrink(code[:899_999]) < 1000 and bm.period_shrink(cases.gen(700_001, "periodic", 9)) < 1000
    lo = plan(cases.gen(600_000, "lowalpha", 2))
    assert lo["np"] and lo["over"][2] > 0 and not lo["spans"]


def test_model_is_fast():
    import time
    x = corpus.enwik_synthetic(899_999, seed=9).tobytes()
    t = time.perf_counter()
    bm.block_plan(x)
    bm.round0(x, True)
    bm.round0(x, False)
    assert time.perf_counter() - t < 4.0
