"""Runs the suffix sort's edge families (tests/bwt_paths_model.py) with BZH_TRACE_ROUNDS=1 under one setting of the path
switches (argv[1]: default | msd | lsd | nomid = BZH_INIT=msd with BZH_MID=0) and prints, on stderr, a line "@@run NAME" in
front of the trace lines of every run.  tests/test_gpu_bwt_edges.py holds the trace to the model; this process only checks
that every block's last column, origin pointer and byte set equal the oracle's (stdout: "mismatches: N", exit code 1 on
any).  A process of its own: the switches are read once per process."""
import os
import sys

mode = sys.argv[1] if len(sys.argv) > 1 else "default"
os.environ["BZH_TRACE_ROUNDS"] = "1"
os.environ.pop("BZH_INIT", None)
os.environ.pop("BZH_MID", None)
if mode in ("msd", "nomid"):
    os.environ["BZH_INIT"] = "msd"
if mode == "lsd":
    os.environ["BZH_INIT"] = "lsd"
if mode == "nomid":
    os.environ["BZH_MID"] = "0"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from banzai_amd import _native as nv  # noqa: E402
from oracle import pyoracle as po  # noqa: E402
from tests import bwt_paths_model as bm  # noqa: E402


def runs():
    """(name, level, max_batch, blocks) for this mode: the same list tests/test_gpu_bwt_edges.py rebuilds"""
    fam = bm.families()
    out = [(name, lvl, mb, blocks) for name, (lvl, mb, blocks) in bm.mixed_batches(fam).items()]
    if mode in ("default", "lsd"):  # one block a batch: the 8 passes (round thresholds at depth 8)
        for k in ("tail_g", "gid8", "five_passes", "quad"):
            out += [(f"{k}/{side}", 9, 8, [fam[k][side]]) for side in (0, 1)]
    if mode == "nomid":  # one block a batch on the bucket-first sort, big lists on the global passes (depth 7)
        out += [(f"gid7/{side}", 9, 8, [fam["gid7"][side]]) for side in (0, 1)]
    if mode == "msd":  # every family block alone on the bucket-first sort: its plan
        out += [(f"{k}/{side}", 9, 1, [fam[k][side]]) for k in sorted(fam) if k not in ("gid8", "five_passes") for side in (0, 1)]
    return out


bad = 0
ctxs = {}
try:
    for name, level, mb, blocks in runs():
        if (level, mb) not in ctxs:
            ctxs[(level, mb)] = nv.Context(0, level, mb)
        sys.stderr.write(f"@@run {name}\n")
        sys.stderr.flush()
        got = ctxs[(level, mb)].bwt_batch(blocks)
        for k, (blk, g) in enumerate(zip(blocks, got)):
            o = po.bwt(blk)
            if not (g[0] == o[0] and g[1] == o[1] and np.array_equal(g[2], o[2])):
                bad += 1
                print("BWT MISMATCH", name, k, len(blk))
finally:
    for c in ctxs.values():
        c.close()
sys.stderr.write("@@run end\n")
print(f"reach {mode}: mismatches: {bad}")
sys.exit(1 if bad else 0)
