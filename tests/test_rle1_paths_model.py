"""CPU: tests/rle1_paths_model.py -- the model of rle1.hip's paths -- against the oracle, on every case of tests/rle1_cases.py.

Per case: the model's block table equals oracle.rle_one iterated over the input (on slices bounded by what a block can consume),
its RLE1 bytes (placed by the emit kernel's offset arithmetic) and its CRCs (folded as crc_range folds them) are the oracle's,
its `open` flags are sound (a block the model calls final does not move when the oracle is given more input), and the record
shows every fact the case was built to reach.  So when the GPU test says "this case drives plan_split through a rejection at
wavefront 14", that is the statement of a model which cuts the oracle's blocks.

REACHED is asserted: it is what the union of all records shows, so a later change of a builder cannot silently lose an edge.
NOT_REACHED, with the reason:
  * wf:start_N -- a speculated start equal to the input's end.  end_from_lim is only asked for lim < total, and then the run it
    stops in holds more canonical bytes than the budget left for it (else the next run start, or the total, would be <= lim
    too), so cut_in_run leaves at least one byte of that run: the start is < N.  The kernel's `sw < N` test covers
    no_origin and past_total, which set sw = N themselves.

The mutant check shows that the cases can tell a wrong kernel from a right one without running a wrong kernel: each of the
model's deliberate single-decision faults makes at least one named case differ from the oracle."""
import collections
import functools

import pytest

from tests import rle1_cases as rc
from tests import rle1_paths_model as pm

NOT_REACHED = {"wf:start_N"}
REACHED = set(pm.FACTS) - NOT_REACHED


def open_unsound(oracle, data, level, blocks, opens):
    """the blocks (of the last three) that the flags call final although more input moves their cut: the input's last byte
    repeated (its last run goes on) and another byte (it ends)"""
    bad = []
    for b in range(max(0, len(blocks) - 3), len(blocks)):
        if opens[b]:
            continue
        off, used, rl = blocks[b]
        for ext in (bytes([data[-1]]) * 2000, bytes([data[-1] ^ 1]) * 8):
            r, _, u = oracle.rle_one(data[off:] + ext, level)
            if (u, len(r)) != (used, rl):
                bad.append(b)
                break
    return bad


def differences(oracle, name, mutant=None, **kw):
    """-> (what of the model's result is not the oracle's, the model's facts)"""
    (_, level, d, want), r = rc.analysed(name, mutant=mutant, **kw)
    oi, oc = rc.oracle_split(oracle, d, level)
    diff = []
    if r.blocks != [x[:3] for x in oi]:
        diff.append("blocks")
    else:
        if r.crcs != [x[3] for x in oi]:
            diff.append("crc")
        if any(r.rle(b) != oc[b] for b in range(len(oc))):
            diff.append("bytes")
        if open_unsound(oracle, d, level, r.blocks, r.open):
            diff.append("open")
        if not r.open[-1]:
            diff.append("last block not open")
    return diff, r.facts, want


@functools.lru_cache(maxsize=None)
def _facts(name):
    from oracle import pyoracle
    diff, facts, want = differences(pyoracle, name)
    return tuple(diff), facts, tuple(pm.unmet(facts, want))


@pytest.mark.parametrize("name", rc.NAMES)
def test_case_is_the_oracles_and_reaches_its_edge(oracle, name):
    diff, _, unmet = _facts(name)
    assert diff == ()
    assert unmet == ()


@pytest.mark.parametrize("level", [1, 9])
def test_residues_at_a_later_boundary_cover_cut_in_run(oracle, level):
    """every class cut_in_run distinguishes, at the third (level 1) and second (level 9) block boundary"""
    u = collections.Counter()
    for name in rc.FAMILIES["residues%d" % level]:
        u.update(_facts(name)[1])
    want = ["cir:k<nf", "cir:k==nf", "cir:ell>=4", "cir:ell<4", "cir:rho0", "cir:rho1", "cir:rho2", "cir:rho3", "cir:rho4",
            "cut:ends_M-1", "cut:ends_M", "sel:fit", "gran:reused", "gran:fresh", "probe:prefix"]
    assert pm.unmet(u, want) == []


def test_ranged_split_and_grid_crc(oracle):
    """plan_split from a block start inside a run to a stop inside wavefront 0's blocks, at the window's block 8 and in wavefront 1;
    the CRCs as crc_tiles (the grid form of plan_crc_range) ranges them"""
    (_, level, d, _), full = rc.analysed("ranged")
    oi, _ = rc.oracle_split(oracle, d, level)
    assert full.blocks == [x[:3] for x in oi]
    assert pm.emitted_before(oi[1][0] - 97_000) > 0 and d[oi[1][0] - 1] == d[oi[1][0]] == 250  # block 1 starts inside the run
    seen = collections.Counter()
    for label, start, stop, lo, hi in rc.ranged_splits(full.blocks):
        r = pm.analyse(d, level, start=start, stop=stop, crc="grid")
        assert r.blocks == full.blocks[lo:hi], label
        assert r.crcs == [x[3] for x in oi[lo:hi]], label
        want = dict(wave0=["wfcut:fin", "reject:stop", "kept:1"], block8=["wfcut:fin", "reject:stop", "kept:2", "wf:spec"],
                    wave1=["wfcut:fin", "reject:stop", "kept:2"], end=["reject:input_done"])[label]
        assert pm.unmet(r.facts, want + ["crc:grid"]) == [], label
        seen.update(r.facts)
    _RANGED.update(seen)


_RANGED = collections.Counter()


def test_grid_crc_of_a_block_that_is_one_enormous_run(oracle):
    """crc_tiles' ranges over a block of 623 tiles of 8 KiB"""
    diff, facts, _ = differences(oracle, "first_run_open", crc="grid")
    assert diff == [] and pm.unmet(facts, ["crc:grid", "crc:tiles>=100", "crc:ranges>1", "crc:ranges1"]) == []


def test_reached_edges(oracle):
    """the union of all records is exactly REACHED"""
    u = collections.Counter()
    for name in rc.NAMES:
        u.update(_facts(name)[1])
    if not _RANGED:
        test_ranged_split_and_grid_crc(oracle)
    u.update(_RANGED)
    got = {f for f in pm.FACTS if u[f]}
    assert got == REACHED, (sorted(REACHED - got), sorted(got - REACHED))
    # rejections at both ends of the window, every probe outcome under both callers
    for f in ("reject_at:mismatch@1", "reject_at:mismatch@14", "kept:15"):
        assert u[f], f


# ---- mutants: faults of the model, never of a kernel ------------------------------------------------------------------------
KILLERS = {
    "probe_le_64": ("probe_full", "probe_full_long_runs"),
    "fit_ignores_lim": ("one_past", "residue_L1_pre-1_run4"),
    "spec_keeps_mismatch": ("spec_reject_w1",),
    "no_ell_clamp": tuple("residue_L1_pre%+d_run6" % p for p in rc.RESIDUE_PRE),
    "open_zero": ("to_end_less", "first_run_open"),
    "emit_no_restart": ("cut_in_long_runs", "ranged"),
    "crc_ragged_last": ("len_8193", "one_past"),
}


@pytest.mark.parametrize("mutant", pm.MUTANTS)
def test_mutant_is_caught(oracle, mutant):
    caught = {}
    for name in KILLERS[mutant]:
        try:
            diff = differences(oracle, name, mutant=mutant)[0]
        except (AssertionError, IndexError, ValueError) as e:  # (a fault may also leave the model without a table)
            diff = [type(e).__name__]
        if diff:
            caught[name] = diff
    assert caught, mutant


def test_every_mutant_has_killers():
    assert set(KILLERS) == set(pm.MUTANTS)
    assert all(n in rc.NAMES for ks in KILLERS.values() for n in ks)
