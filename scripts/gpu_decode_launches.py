"""The decoder's launch sequence, for comparing two builds of the library kernel by kernel:
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/gpu_decode_launches.py run
      one full decode, one index build, one sync index build (interval 2: four points a block), one range decode and one sync
      range decode of a 12-block level-1 stream on Context(0, 1, 4) -- three batches, the range from the middle of block 1 to the
      middle of block 9; then, both with the sync points, one decode_ranges call of three ranges (block 2 whole, block 3 cut, two
      pieces of block 6) and, over a record table of the spaces, one decode_records call of three (block 2 cut, block 3 whole,
      block 4 cut, two pieces of block 6);
  python scripts/gpu_decode_launches.py list DIR > launches.txt
      the kernels of that trace in start order, one line each: name, grid, workgroup.
BZH_LIB names the library to load (default: the tree's)."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run():
    import bz2
    from banzai_amd import _native as nv
    from tests import cases
    truth = cases.gen(1_150_000, "text", 3)
    s = bz2.compress(truth, 1)
    with nv.Context(0, 1, 4) as c:
        assert c.decode(s, size_hint=len(truth)) == truth
        ent, total, _ = c.decode_index(s)
        assert len(ent) == 12 and total == len(truth)
        ent2, pts, _, _ = c.decode_index_sync(s, 2)  # (a block of this text has 10 groups: 4 points each)
        assert ent2.tobytes() == ent.tobytes() and len(pts) == 4 * len(ent)
        mid = lambda k: int(ent[k]["out_off"]) + int(ent[k]["out_len"]) // 2
        off, n = mid(1), mid(9) - mid(1)
        assert c.decode_range(s, ent, off, n) == truth[off:off + n]
        assert c.decode_range_sync(s, ent, pts, off, n) == truth[off:off + n]
        b, n = (lambda k: int(ent[k]["out_off"])), (lambda k: int(ent[k]["out_len"]))
        ranges = [(b(2), n(2) + 100), (b(6) + 10, 100), (mid(6), 100)]
        blob, offs, lens = c.decode_ranges(s, ent, ranges, pts)
        assert [blob[o:o + m] for o, m in zip(offs, lens)] == [truth[o:o + m] for o, m in ranges]
        ent3, _, cum, nrec, _, _ = c.decode_index_records(s, 0, 32)
        assert ent3.tobytes() == ent.tobytes()
        words = truth.split(b" ")  # record r = words[r] and its space
        assert nrec == len(words)
        recs = [(int(cum[2]) + 5, int(cum[4] - cum[2])), (int(cum[6]) + 10, 3), (int(cum[6]) + 100, 3)]
        blob, offs, lens = c.decode_records(s, ent, cum, recs, pts, delim=32)
        assert [blob[o:o + m] for o, m in zip(offs, lens)] == [b"".join(w + b" " for w in words[f:f + k]) for f, k in recs]
    print(f"gpu_decode_launches: 7 calls over {len(ent)} blocks, {len(pts)} sync points")


def listing(trace_dir):
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        print(f'{r["Kernel_Name"]} grid {r["Grid_Size_X"]}x{r["Grid_Size_Y"]}x{r["Grid_Size_Z"]} workgroup {r["Workgroup_Size_X"]}')


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) == 3 and sys.argv[1] == "list":
        listing(sys.argv[2])
    else:
        sys.exit(__doc__)
