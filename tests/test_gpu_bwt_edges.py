"""The suffix sort at the edges of its path choices (tests/bwt_paths_model.py): every family block bit-exact against the
oracle on the 8 passes and in batches large enough for the bucket-first sort, mixed streams at levels 9 and 2, and -- in
child processes with BZH_TRACE_ROUNDS=1 (scripts/gpu_bwt_reach.py) -- the trace of each run equal to what the model says
the device decides: bucket-first / 8-pass blocks, units, oversized buckets and tiles per level, levels 2-5 run or
skipped, spans, near-periodic blocks, big lists on ranks, four or five passes, the depth x4 form."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from banzai_amd import corpus
from tests import bwt_paths_model as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fam():
    return bm.families()


def _same(g, o):
    return g[0] == o[0] and g[1] == o[1] and np.array_equal(g[2], o[2])


@pytest.mark.gpu
def test_family_blocks_on_the_8_passes(native, oracle, fam):
    """every family block alone (a batch of one: the 8 passes)"""
    with native.Context(0, 9, 8) as ctx:
        for name, pair in fam.items():
            for side, blk in enumerate(pair):
                assert _same(ctx.bwt(blk), oracle.bwt(blk)), (name, side, len(blk))


@pytest.mark.gpu
def test_family_blocks_batched(native, oracle, fam):
    """all family blocks in batches of 16 (the default decisions: bucket-first where the plan allows it), in two orders"""
    blocks = [b for pair in fam.values() for b in pair]
    want = [oracle.bwt(b) for b in blocks]
    perm = np.random.default_rng(5).permutation(len(blocks))
    with native.Context(0, 9, 16) as ctx:
        for order in (np.arange(len(blocks)), perm):
            got = ctx.bwt_batch([blocks[i] for i in order])
            for k, i in enumerate(order):
                assert _same(got[k], want[i]), (int(i), len(blocks[i]))


@pytest.mark.gpu
@pytest.mark.parametrize("level", [9, 2])
def test_mixed_streams(native, oracle, level):
    """the mixed batch lists as whole streams (RLE1, cut into blocks of the level, then the sort), padded with text to at
    least 12 blocks per batch"""
    fam = bm.families()
    lvl, mb, blocks = bm.mixed_batches(fam)["mixed9a" if level == 9 else "mixed2"]
    body = b"".join(blocks)
    need = 12 * (100000 * level) + 50_000
    text = corpus.enwik_synthetic(max(0, need - len(body)), seed=31).tobytes()
    data = body[:len(body) // 2] + text + body[len(body) // 2:]
    with native.Context(0, level, mb) as ctx:
        assert ctx.encode(data) == oracle.encode(data, level)


# ---- reach: the trace against the model ------------------------------------------------------------------------------

_INIT = re.compile(r"initial sort: (\d+) blocks bucket-first, (\d+) blocks 8-pass; (\d+) units; .* oversized buckets per level "
                   r"(\d+) (\d+) (\d+) (\d+) (\d+) \(tiles (\d+) (\d+) (\d+) (\d+) (\d+)\)")
_RULE = re.compile(r"initial sort: 0 blocks bucket-first, (\d+) blocks 8-pass \(the batch rule\)")
_LEVELS = re.compile(r"initial sort: levels 2-5 (ran|skipped)")
_BLOCK = re.compile(r"initial sort, block (\d+): (bucket-first|8-pass), (\d+) units, spans (\d+)")
_ROUND = re.compile(r"round (\d+) h<=(\d+) unresolved=(\d+)  S blocks=(\d+) \(max (\d+)\)  A blocks=(\d+) \(max (\d+), (on ranks|on group numbers)\)"
                    r"  T blocks=(\d+) \(quad (\d+), max (\d+)\)")
_PASSES = re.compile(r"round (\d+): global passes over big lists of at most (\d+) records: (\d) passes")
_PERIOD = re.compile(r"block (\d+): near-periodic, sorted as (\d+) periods of (\d+) bytes \+ (\d+)")


def _runs(stderr):
    out, name = {}, None
    for line in stderr.splitlines():
        if line.startswith("@@run "):
            name = line[6:].strip()
            out[name] = []
        elif name is not None and line.startswith("[bzhip]"):
            out[name].append(line)
    return out


def _batches(lines):
    """the initial-sort records of a run, one per batch, in order"""
    out = []
    for ln in lines:
        m = _INIT.search(ln)
        if m:
            v = [int(x) for x in m.groups()]
            out.append({"msd": True, "new": v[0], "old": v[1], "units": v[2], "over": [0] + v[3:8], "tiles": [0] + v[8:13], "blocks": []})
            continue
        m = _RULE.search(ln)
        if m:
            out.append({"msd": False, "old": int(m.group(1))})
            continue
        m = _LEVELS.search(ln)
        if m:
            out[-1]["deeper"] = m.group(1) == "ran"
            continue
        m = _BLOCK.search(ln)
        if m:
            out[-1]["blocks"].append((m.group(2) == "bucket-first", int(m.group(3)), int(m.group(4)) != 0))
    return out


def _rounds(lines):
    r, p = {}, {}
    for ln in lines:
        m = _ROUND.search(ln)
        if m and int(m.group(1)) not in r:
            v = m.groups()
            r[int(v[0])] = {"h": int(v[1]), "S": int(v[3]), "A": int(v[5]), "maxA": int(v[6]), "on_ranks": v[7] == "on ranks",
                            "T": int(v[8]), "quad": int(v[9]), "maxT": int(v[10])}
        m = _PASSES.search(ln)
        if m:
            p[int(m.group(1))] = (int(m.group(2)), int(m.group(3)))
    return r, p


def _check_plan(name, lines, blocks, level, mb, init):
    got = _batches(lines)
    want = bm.batch_plans(blocks, level, mb, init)
    assert len(got) == len(want), (name, lines)
    for k, (g, w) in enumerate(zip(got, want)):
        where = (name, k)
        assert g["msd"] == w["msd"], where
        assert g["old"] == w["old"], where
        if not w["msd"]:
            continue
        assert (g["new"], g["units"], g["over"], g["tiles"], g["deeper"]) == (w["new"], w["units"], w["over"], w["tiles"], w["deeper"]), (where, g, w)
        assert g["blocks"] == [(p["np"], p["units"] if p["np"] else 0, p["spans"] if p["np"] else False) for p in w["plans"]], where
    # near-periodic blocks: as many as the model shrinks, to the model's length
    shr = sorted(bm.period_shrink(b) for b in blocks if bm.period_shrink(b) != len(b))
    seen = sorted(int(m.group(2)) * int(m.group(3)) + int(m.group(4)) for m in map(_PERIOD.search, lines) if m)
    assert seen == shr, (name, seen, shr)


def _check_round0(name, lines, blk, msd):
    w = bm.round0(blk, msd)
    r, p = _rounds(lines)
    g = r[0]
    assert g["h"] == w["h"], name
    assert g["A"] == (1 if w["big_records"] and not w["sweep"] else 0), (name, g, w)
    if g["A"]:
        assert g["maxA"] == w["big_records"], (name, g, w)
        assert g["on_ranks"] == w["on_ranks"], (name, g, w)
    if not msd:
        assert g["quad"] == (1 if w["quad"] else 0), (name, g, w)
        if g["T"]:
            assert g["maxT"] == w["small_records"], (name, g, w)
    return w, r, p


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["default", "msd", "lsd", "nomid"])
def test_trace_reaches_each_edge(native, mode):
    """scripts/gpu_bwt_reach.py under one setting of the switches: its bytes equal the oracle's, and its trace equals the
    model on both sides of every edge the run covers"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "gpu_bwt_reach.py"), mode], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "mismatches: 0" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    runs = _runs(r.stderr)
    fam = bm.families()
    init = {"default": "default", "lsd": "lsd", "msd": "msd", "nomid": "msd"}[mode]
    for name, (lvl, mb, blocks) in bm.mixed_batches(fam).items():
        _check_plan(name, runs[name], blocks, lvl, mb, init)
    if mode in ("default", "lsd"):
        w = [_check_round0(f"tail_g/{s}", runs[f"tail_g/{s}"], fam["tail_g"][s], False)[0] for s in (0, 1)]
        assert [x["big_records"] > 0 for x in w] == [False, True]
        w = [_check_round0(f"gid8/{s}", runs[f"gid8/{s}"], fam["gid8"][s], False)[0] for s in (0, 1)]
        assert [x["on_ranks"] for x in w] == [False, True]
        for s, want in ((0, (250000, 4)), (1, (250001, 5))):
            _, _, p = _check_round0(f"five_passes/{s}", runs[f"five_passes/{s}"], fam["five_passes"][s], False)
            assert p.get(1) == want, (s, p)
        w = [_check_round0(f"quad/{s}", runs[f"quad/{s}"], fam["quad"][s], False)[0] for s in (0, 1)]
        assert [x["quad"] for x in w] == [True, False]
    if mode == "nomid":
        w = [_check_round0(f"gid7/{s}", runs[f"gid7/{s}"], fam["gid7"][s], True)[0] for s in (0, 1)]
        assert [x["on_ranks"] for x in w] == [False, True]
    if mode == "msd":
        for k in fam:
            if k in ("gid8", "five_passes"):
                continue
            for s in (0, 1):
                _check_plan(f"{k}/{s}", runs[f"{k}/{s}"], [fam[k][s]], 9, 1, "msd")
