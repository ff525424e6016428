"""Inputs that drive the first encoder stage (banzai_amd/csrc/rle1.hip: run tables, the closed-form cut, plan_split's
speculative windows, the block CRCs, rle1_emit_kernel) to its path edges, each with the facts it was built to reach -- facts
of tests/rle1_paths_model.py's record, so the CPU test and the GPU test can both show that a builder still gets there before
anything is compared.  The model, not the builder's author, says what a case reaches: parameters marked "(search)" were found
by running the model over a range of candidates; the search is not repeated here, its result is asserted.

A case is (name, level, data, want); `want` is a list for rle1_paths_model.unmet().  FAMILIES groups the names; case(name)
builds one (cached), analysed(name) adds the model's Result.  LARGE names the cases above 2.5 MB, each of which needs its
size: wavefront w of plan_split speculates only when more than 8 w blocks lie ahead of the window (so "15 kept, then a second
window" and "rejected at wavefront 14" want 121 and 113 blocks of 99,999 bytes), a block starts on a run longer than its
budget from 5,100,000 equal bytes on at level 1, and plan_carries / plan_tc carry from one chunk of 16,384 tiles to the next
from 64 MiB on.
"""
import functools

import numpy as np

from tests import rle1_paths_model as pm

M1, M9 = 99_999, 899_999
RUNS = (3, 4, 5, 254, 255, 256, 258, 259, 510, 514)
NEAR = (-3, -2, -1, 0, 1, 2, 3)
LENGTHS = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 8224, 16384, 12303)
RESIDUE_PRE = tuple(range(-8, 3))
RESIDUE_RUNS = {1: (3, 4, 5, 6, 255, 256, 259, 600), 9: (3, 4, 256, 259)}


def lit(n, seed):
    """n bytes 1..199 without two equal neighbours: one canonical RLE1 byte each"""
    rng = np.random.default_rng(seed)
    return ((np.cumsum(rng.integers(1, 199, n)) % 199) + 1).astype(np.uint8).tobytes()


def run(n, b=250):
    return bytes([b]) * n


# ---- speculation ------------------------------------------------------------------------------------------------------------
def _spec_kept15():
    """122 blocks of run-free bytes: every wavefront's start is right, the second window begins behind 120 kept blocks"""
    return 1, lit(121 * M1 + 54_321, 1), ["kept:15", "reject:none", "windows:2", "wf:spec", "wfcut:full", "crc:pos>=64",
                                          ("wf:spec", 14), "!reject:mismatch"]


def _spec_reject(at_block, blocks, w, back):
    """run-free bytes but for a run of six that begins `back` bytes before the end of block `at_block`'s budget.  back = 4: the
    block ends on M - 1 (three literals, the fourth would want its count byte).  back = 3: it ends on M, but the three bytes
    left of the run are literals again (six bytes where the canonical stream has five).  Either way every later start lies
    a byte off what origin + j M says."""
    d = bytearray(lit(blocks * M1 + 7_000, 2 + w))
    p = (at_block + 1) * M1 - back
    d[p:p + 6] = run(6)
    return 1, bytes(d), ["reject_at:mismatch@%d" % w, "cut:ends_M-1" if back == 4 else "!cut:ends_M-1", "wf:spec"]


def _spec_short():
    """ten blocks: wavefront 1 cuts two and the input ends, wavefronts 2.. start past the total"""
    return 1, lit(9 * M1 + 500, 5), ["wf:spec", "wf:past_total", "wfcut:input_ended", "wfcut:none", "reject:input_done", "kept:2"]


# ---- the branches of a cut -----------------------------------------------------------------------------------------------------
FIRST_RUN = 255 * 20_000  # canon_len = 100,000 > M: the shortest run a level-1 block cannot take whole


def _first_run_then_text():
    """a block starts on a run longer than its budget (the input's first), no origin for the window: wavefronts 1..14 cut nothing,
    and eight blocks behind it the window ends on an empty wavefront"""
    d = run(FIRST_RUN + 12_345) + lit(9 * M1, 6)
    return 1, d, ["cut:first_run", "wf:no_origin", "reject:empty", "crc:tiles>=100", "obase:first_run", "open:0"]


def _first_run_open():
    """the whole input is one run a little longer than the budget: the cut could move if more of the run followed"""
    return 1, run(FIRST_RUN + 100), ["cut:first_run", ("open:0", 0), "cut:to_end_lt", "next:nrsg"]


def _first_run_later():
    """60 literal bytes, then a run of 2 x 5,100,000: block 0 is cut inside the run by end_from_lim, block 1 starts on what is
    left of it -- still more than a budget"""
    return 1, lit(60, 7) + run(2 * FIRST_RUN) + lit(1000, 8), ["cut:first_run", "cut:end_from_lim", "sel:rsg", "!wf:no_origin"]


def _to_end_equal():
    return 1, lit(M1, 9), ["cut:to_end_eq", ("cut:to_end_eq", 1)]


def _to_end_less():
    return 1, lit(M1 - 1, 9), ["cut:to_end_lt"]


def _one_past():
    return 1, lit(M1 + 1, 9), ["cut:end_from_lim", "cut:ends_M", "cut:to_end_lt"]


# ---- end_from_lim's probe -----------------------------------------------------------------------------------------------------------
def _runs_of(length, n, seed):
    """runs of `length` bytes, neighbours different"""
    v = ((np.cumsum(np.random.default_rng(seed).integers(1, 199, n // length + 1)) % 199) + 1).astype(np.uint8)
    return np.repeat(v, length)[:n].tobytes()


def _probe_full():
    """runs of 16: a tile emits 1,280 bytes, the budget ends 78 tiles on -- beyond the 64 tiles of the probe"""
    return 1, _runs_of(16, 700_000, 10), ["probe:full", "rounds:1", "sel:fit"]


def _probe_full_long_runs():
    """runs of 9,000: a tile emits 40 bytes, every other tile has no run start; the 64-ary search runs over hundreds of tiles"""
    return 1, _runs_of(9000, 2_300_000, 11) + lit(120_000, 12), ["probe:full", "sel:fit", "tile:no_start", "tile:other"]


def _probe_miss_level9():
    """runs of four: a tile emits 5,120 bytes, the literal-text guess lies 4 tiles past the tile where a level-9 budget ends"""
    return 9, _runs_of(4, 1_000_000, 13), ["probe:miss", "rounds:2"]


def _probe_miss_speculation():
    """the same at level 1, where only a speculated start looks far enough ahead (wavefront 2: 16 budgets)"""
    return 1, _runs_of(4, 2_000_000, 14), ["probe:miss", "wf:spec"]


def _cut_in_long_runs():
    """runs of 70,000 and short ones: cuts inside runs that cover whole granules (rsg), blocks that start inside a run"""
    d = lit(97_000, 17) + run(300_000) + lit(92_000, 18) + run(200_000, 251) + lit(120_000, 19) + run(70_000, 252) + lit(50_000, 20)
    return 1, d, ["sel:rsg", "sel:fit", "obase:first_run", "cir:k<nf", "gran:reused", "gran:fresh"]


def _last_granule():
    """(search) a run in front shifts the first cut into the last granule of the padded last tile, and the rest is one run: the
    next run start comes from nrsg[ngran]"""
    d = run(2400, 7) + lit(M1 - 50, 15) + run(30)
    return 1, d, ["next:nrsg_end", "next:nrsg"]


def _tile_edge_block():
    """(search) block 0 ends two bytes into a tile: a tile with nothing but a ragged tail, the next block's first tile with a
    head outside the block"""
    d = run(2453, 7) + lit(M1 - 50 + 5000, 16)
    return 1, d, ["nwords:0", "emit:head_outside", "emit:tail_outside"]


# ---- thread, wavefront, granule and tile seams -------------------------------------------------------------------------------------
def _seams(boundary, slot):
    """every run length of RUNS placed so that its 4th byte (kk == 3) and, if it has one, its 255th (kk == 254, the full chunk's
    count byte) falls 0..3 bytes before and after a multiple of `boundary` that is no multiple of the next larger boundary;
    run-free bytes between them, so literal-only and slow wavefronts meet inside tiles"""
    place = [(L, kk, dd) for L in RUNS for kk in (3, 254) if L > kk for dd in NEAR]
    place += [(3, 2, dd) for dd in NEAR]  # (a run of three has no 4th byte: its last one)
    d = bytearray(lit(slot * (len(place) + 1), boundary))
    for k, (L, kk, dd) in enumerate(place):
        at = slot * (k + 1) + boundary  # (slot is a multiple of 4096 or of 2048: `at` is a multiple of `boundary` only)
        assert at % boundary == 0 and (boundary == 4096 or at % (boundary * 4) != 0)
        s = at + dd - kk
        d[s:s + L] = run(L)
    return 1, bytes(d), ["wave:slow", "wave:literal", "emit:mixed_waves"]


def _head_run(o, L):
    """a run of L at input offset o = 0..3: has_run_of_four without three bytes to look back on"""
    return 1, lit(o, 20 + o) + run(L) + lit(50, 30 + L), ["wave:slow" if L >= 4 else "!wave:slow", "cut:to_end_lt"]


def _length(n):
    """n bytes of short runs: ragged last thread, granule and tile"""
    from tests import cases
    return 1, cases.gen(n, "shortruns", 4), ["cut:to_end_lt", ("windows:1", 1)]


# ---- cut residues at a later block boundary ------------------------------------------------------------------------------------------
def _residue(level, pre, runlen):
    """tests/cases.py's boundary_cases behind whole blocks of run-free bytes (two at level 1, one at level 9): the run straddles
    the end of the third (second) block, whose budget is counted from a canonical offset deep inside the tables"""
    M = 100_000 * level - 1
    lead = (2 if level == 1 else 1) * M
    d = lit(lead + M + pre, 100 * level + pre + 9 + runlen) + run(runlen) + lit(3000, runlen)
    return level, d, ["cut:end_from_lim", "!cut:first_run"]


def _chunk_seam():
    """64 MiB and a little at level 9: a run from the first tiles to beyond tile 16,384 (both seams of plan_carries: the forward
    chunks are counted from the first tile, the backward ones from the last), run-free bytes behind it so that a cut falls
    where tc is carry + in-chunk scan.  Block 1 starts on 21 MB of the run, block 0 is cut inside it."""
    head, tail = lit(3000, 40), lit(1_300_000, 41)
    n = (64 << 20) + 40_000
    d = head + run(n - len(head)) + tail
    return 9, d, ["chunks:2", "seam:fwd_run", "seam:bwd_run", "cut:end_from_lim", "sel:rsg", "obase:first_run", "crc:tiles>=100"]


def _ranged():
    """block 0 is cut inside a run of 300,000, so block 1 -- where the ranged splits of the tests start -- begins inside it; 19
    blocks of run-free bytes behind it: a window that starts at block 1 has wavefront 1 begin at block 9"""
    return 1, lit(97_000, 50) + run(300_000) + lit(19 * M1, 51), ["sel:rsg", "wf:spec", "obase:first_run", "kept:2"]


def ranged_splits(blocks):
    """(label, start, stop, lo, hi) -- the split lists blocks[lo:hi] -- for the case "ranged": from block 1 to the first block that starts
    at or after a stop inside wavefront 0's blocks, exactly at the window's block 8, inside wavefront 1's blocks, and beyond
    the input"""
    off = [b[0] for b in blocks]
    out = []
    for label, stop in (("wave0", off[4] + 5), ("block8", off[9]), ("wave1", off[12] + 1), ("end", None)):
        last = len(off) - 1 if stop is None else min(k for k in range(len(off)) if off[k] >= stop)
        out.append((label, off[1], stop, 1, last + 1))
    return out


def oracle_split(oracle, data, level):
    """oracle.rle_one iterated over `data` -> ([(in_off, in_len, rle_len, crc)], [RLE1 bytes]).  Every call gets a slice, not the
    rest of the input: rle_one reads forward and looks at most 256 bytes ahead of what it consumes, so a block that ends 300
    bytes or more before the end of its slice is the block the whole rest would give (else the slice is widened)."""
    M = 100_000 * level - 1
    off, res, chunks = 0, [], []
    while off < len(data):
        ln = 2 * M
        while True:
            sl = data[off:off + ln]
            r, crc, used = oracle.rle_one(sl, level)
            if off + len(sl) >= len(data) or used + 300 <= len(sl):
                break
            ln *= 4
        res.append((off, used, len(r), crc))
        chunks.append(r)
        off += used
    return res, chunks


# ---- registry ------------------------------------------------------------------------------------------------------------------------
_BUILDERS = {}
FAMILIES = {}


def _add(family, name, fn, *args):
    _BUILDERS[name] = (fn, args)
    FAMILIES.setdefault(family, []).append(name)


_add("large", "spec_kept15_second_window", _spec_kept15)
_add("large", "spec_reject_w14", _spec_reject, 108, 114, 14, 3)
_add("large", "first_run_then_text", _first_run_then_text)
_add("large", "first_run_open", _first_run_open)
_add("large", "first_run_later", _first_run_later)
_add("large", "chunk_seam_level9", _chunk_seam)
_add("split", "spec_reject_w1", _spec_reject, 3, 12, 1, 4)
_add("split", "spec_short", _spec_short)
_add("split", "ranged", _ranged)
_add("cut", "to_end_equal", _to_end_equal)
_add("cut", "to_end_less", _to_end_less)
_add("cut", "one_past", _one_past)
_add("cut", "cut_in_long_runs", _cut_in_long_runs)
_add("cut", "last_granule", _last_granule)
_add("cut", "tile_edge_block", _tile_edge_block)
_add("probe", "probe_full", _probe_full)
_add("probe", "probe_full_long_runs", _probe_full_long_runs)
_add("probe", "probe_miss_level9", _probe_miss_level9)
_add("probe", "probe_miss_speculation", _probe_miss_speculation)
for _b, _slot in ((16, 2048), (64, 2048), (1024, 4096), (4096, 8192)):
    _add("seams", "seams_%d" % _b, _seams, _b, _slot)
for _o in range(4):
    for _L in RUNS:
        _add("head", "head_o%d_L%d" % (_o, _L), _head_run, _o, _L)
for _n in LENGTHS:
    _add("lengths", "len_%d" % _n, _length, _n)
for _lv in (1, 9):
    for _pre in RESIDUE_PRE:
        for _L in RESIDUE_RUNS[_lv]:
            _add("residues%d" % _lv, "residue_L%d_pre%+d_run%d" % (_lv, _pre, _L), _residue, _lv, _pre, _L)

NAMES = [n for fam in FAMILIES.values() for n in fam]
LARGE = FAMILIES["large"]
SMALL = [n for n in NAMES if n not in LARGE]  # at most 2.5 MB each


@functools.lru_cache(maxsize=8)
def case(name):
    fn, args = _BUILDERS[name]
    level, data, want = fn(*args)
    assert (len(data) <= 2_500_000) == (name not in LARGE), (name, len(data))
    return name, level, data, want


def analysed(name, **kw):
    """-> (case, model Result)"""
    c = case(name)
    return c, pm.analyse(c[2], c[1], **kw)
