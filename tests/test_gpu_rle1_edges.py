"""GPU (-m gpu): the first encoder stage -- plan_starts, plan_carries, plan_granules, plan_tc, cut_block_to / end_from_lim /
cut_in_run under plan_split's speculative windows and under plan_many_split, crc_range under crc_tiles_flat and crc_tiles,
rle1_emit_kernel -- driven to every path edge by the cases of tests/rle1_cases.py and held to the oracle block for block and
byte for byte.

Before a case goes to the GPU the test asserts, from the record of tests/rle1_paths_model.py, that it reaches the edges it was
built for; tests/test_rle1_paths_model.py shows on the CPU that the model which says so cuts the oracle's blocks.  Then
rle1_split must give the oracle's (in_off, in_len, rle_len, crc) and RLE1 bytes per block, plan_open the model's flags, and
-- for the cases of 2.5 MB and less -- encode the oracle's stream.

Reached (figures from the model's records):
  * plan_split: 15 wavefronts kept and a second window behind 120 blocks (122 blocks, 12.2 MB); a mismatch at wavefront 1 (a
    block that ends on M - 1) and at wavefront 14 (a block that ends on M but leaves three literals of its run); starts that
    are speculated, without origin, past the total; wavefronts that cut 8 blocks, fewer because the input ends, none; windows
    that end on input_done, empty, mismatch, stop and with all 15 kept; ranged splits from a block start inside a run to a
    stop inside wavefront 0's blocks, exactly at the window's block 8 and inside wavefront 1's.
  * cut_block_to: a block that starts on a run longer than its budget (5,100,000 bytes at level 1, at the input's start, at
    a later block start, and open at the input's end); everything fits, with and
    without equality; end_from_lim with the probe's three outcomes (a prefix; all 64 tiles, then 1, 2 and 3 rounds of the
    search; a miss -- at level 9 by a cut, at level 1 by a speculated start 16 budgets ahead), fit and rsg, the granule reused
    and fresh, the next run start from the granule, from nrsg[g + 1] and from nrsg[ngran]; every class of cut_in_run at the
    third (level 1) and second (level 9) block boundary.
  * tables: tiles without a run start and with one at byte 0, literal-only and slow wavefronts in one tile, run lengths 3 ..
    514 with their 4th and 255th byte 0..3 bytes before and after multiples of 16, 64, 1,024 and 4,096 and at input offsets
    0..3, inputs of 1 .. 16,384 bytes around every thread, granule and tile size, two chunks of 16,384 tiles with a run across
    both seams of plan_carries.
  * emit: the three obase branches, output misaligned by 0..3, a tile of fewer than four bytes, heads and tails outside the
    block.  CRC: ragged and whole pieces and tiles, blocks of one and of more than 600 tiles, more than 64 blocks, flat and grid form.
Not reached: a speculated start equal to the input's end (tests/test_rle1_paths_model.py says why it cannot be)."""
import numpy as np
import pytest

from tests import rle1_cases as rc
from tests import rle1_paths_model as pm

pytestmark = pytest.mark.gpu


def _ctx(request, level):
    return request.getfixturevalue("ctx1" if level == 1 else "ctx9")


def _check(oracle, request, name, stream=True):
    (_, level, d, want), r = rc.analysed(name)
    assert pm.unmet(r.facts, want) == [], name  # the builder still reaches its edges
    ctx = _ctx(request, level)
    oi, oc = rc.oracle_split(oracle, d, level)
    assert r.blocks == [x[:3] for x in oi], name  # ... and the model that says so cuts the oracle's blocks
    infos, chunks = ctx.rle1_split(d)
    assert infos == oi, name
    assert ctx.plan_open() == r.open, name
    assert len(chunks) == len(oc) and all(a == b for a, b in zip(chunks, oc)), name
    if stream:
        assert ctx.encode(d) == oracle.encode(d, level), name
    return r


@pytest.mark.parametrize("name", rc.FAMILIES["split"] + rc.FAMILIES["cut"] + rc.FAMILIES["probe"] + rc.FAMILIES["seams"])
def test_split_cut_probe_and_seam_edges(oracle, request, name):
    _check(oracle, request, name)


@pytest.mark.parametrize("o", range(4))
def test_runs_at_the_head_of_the_input(oracle, request, o):
    for L in rc.RUNS:
        _check(oracle, request, "head_o%d_L%d" % (o, L))


def test_input_lengths(oracle, request):
    for name in rc.FAMILIES["lengths"]:
        _check(oracle, request, name)


@pytest.mark.parametrize("pre", rc.RESIDUE_PRE)
@pytest.mark.parametrize("level", [1, 9])
def test_cut_residues_at_a_later_boundary(oracle, request, level, pre):
    for L in rc.RESIDUE_RUNS[level]:
        _check(oracle, request, "residue_L%d_pre%+d_run%d" % (level, pre, L))


@pytest.mark.parametrize("name", rc.LARGE)
def test_large_cases(oracle, request, name):
    """each needs its size (tests/rle1_cases.py); RLE1 and CRCs only, no stream"""
    r = _check(oracle, request, name, stream=False)
    if name == "spec_kept15_second_window":
        assert [w["kept"] for w in r.windows] == [15, 1] and r.windows[0]["nb"] == 120
    if name == "spec_reject_w14":
        assert (r.windows[0]["kept"], r.windows[0]["reject"]) == (14, "mismatch")


def test_ranged_split_and_grid_crc(oracle, request):
    """plan_tables_device + plan_split_device(start, stop) + plan_crc_range: the split from a block start inside a run, to stops
    inside wavefront 0's blocks, at the window's block 8 and inside wavefront 1's; the CRCs by crc_tiles, over sub-ranges"""
    import torch
    (_, level, d, _), full = rc.analysed("ranged")
    ctx = _ctx(request, level)
    oi, _ = rc.oracle_split(oracle, d, level)
    assert full.blocks == [x[:3] for x in oi]
    n = len(d)
    d_in = torch.from_numpy(np.frombuffer(d + b"\0" * 16, dtype=np.uint8).copy()).to("cuda")
    ctx.plan_tables_device(d_in.data_ptr(), n)
    for label, start, stop, lo, hi in rc.ranged_splits(full.blocks):
        r = pm.analyse(d, level, start=start, stop=stop, crc=None, tiles=False)
        assert r.blocks == full.blocks[lo:hi], label
        assert pm.unmet(r.facts, ["reject:input_done"] if stop is None else ["wfcut:fin", "reject:stop"]) == [], label
        nb = ctx.plan_split_device(start, stop, crc=False)
        got = ctx.plan_blocks()
        assert nb == hi - lo and [b[:3] for b in got] == [x[:3] for x in oi[lo:hi]], label
        assert all(b[3] == 0 for b in got), label
        assert ctx.plan_open() == r.open, label
        mid = nb // 2
        assert ctx.plan_crc_range(mid, nb) == [x[3] for x in oi[lo + mid:hi]], label
        assert [b[3] for b in ctx.plan_blocks()[:mid]] == [0] * mid, label
        assert ctx.plan_crc_range(0, mid) == [x[3] for x in oi[lo:lo + mid]], label
        assert ctx.plan_blocks() == oi[lo:hi], label


def test_grid_crc_of_a_block_that_is_one_enormous_run(oracle, request):
    """plan without CRCs, then plan_crc_range: crc_tiles over a block of 623 tiles (78 ranges of 64 KiB) beside one of one tile"""
    import torch
    (_, level, d, _), r = rc.analysed("first_run_open", crc="grid")
    assert pm.unmet(r.facts, ["crc:grid", "crc:tiles>=100", "crc:ranges>1", "crc:ranges1"]) == []
    ctx = _ctx(request, level)
    oi, _ = rc.oracle_split(oracle, d, level)
    assert r.crcs == [x[3] for x in oi]
    d_in = torch.from_numpy(np.frombuffer(d + b"\0" * 16, dtype=np.uint8).copy()).to("cuda")
    got = ctx.plan_device(d_in.data_ptr(), len(d), crc=False)
    assert got == [x[:3] + (0,) for x in oi]
    assert ctx.plan_crc_range(0, len(got)) == [x[3] for x in oi]
    assert ctx.plan_device(d_in.data_ptr(), len(d)) == oi  # the flat form, through the device entry point


MANY = ("cut_in_long_runs", "tile_edge_block", "last_granule", "probe_full", "one_past", "residue_L1_pre-4_run6",
        "probe_miss_level9", "first_run_open")


@pytest.mark.parametrize("name", MANY)
def test_one_input_among_many(oracle, request, name):
    """plan_many_device: cut_block_to with a guard standing in for n -- the case between small neighbours that end and begin
    with the case's first and last byte"""
    import torch
    _, level, d, _ = rc.case(name)
    ctx = _ctx(request, level)
    items = [bytes([d[0]]) * 5, d, bytes([d[-1]]) * 300, b"", rc.lit(1000, 1), bytes([d[0]]) * 4]
    cat = b"".join(items)
    d_in = torch.from_numpy(np.frombuffer(cat + b"\0" * 16, dtype=np.uint8).copy()).to("cuda")
    got = ctx.plan_many_device(d_in.data_ptr(), [len(x) for x in items])
    want, at = [], 0
    for x in items:
        want += [(o + at, ln, r, c) for (o, ln, r, c) in rc.oracle_split(oracle, x, level)[0]]
        at += len(x)
    assert got == want
