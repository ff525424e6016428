"""bzh_decode_ranges_device beside a loop of bzh_decode_range_device on cuda:0: python scripts/gpu_ranges.py [out.json]
Everything resident in HBM, best of 3 after a warm-up, every step a child process under a time limit of its own; the first that
fails ends the script.  Every step compares what it wrote byte for byte.  The input is the 100 MB level-9 headline text.
  loop      256 seeded 4 KiB reads, one bzh_decode_range_device each -- the yardstick: existing code
  ranges    the same 256 reads in one bzh_decode_ranges_device
  sync      the same with sync points at interval 256
  decode    bzh_decode_device of the whole input -- the ceiling when every block is touched
  pieces    4,096 reads of 256 bytes inside one block in one bzh_decode_ranges_device: unrle_walk_pieces.  With
            $BZH_EXPERIMENTS_LIB naming a build made with -DBZH_EXPERIMENTS the step runs a second time on that build with
            BZH_RANGES_WIN=1, which launches unrle_walk_win over the pieces instead, a grid row each
The script fails if `ranges` is not below `loop`.  Writes the JSON."""
import json
import os
import random
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, LEVEL, REPS = 100_000_000, 9, 3
READS, READ = 256, 4096
SMALL, SMALL_READ = 4096, 256
STEPS = ("loop", "ranges", "sync", "decode", "pieces")


def child(step):
    import torch
    sys.path.insert(0, ROOT)
    from banzai_amd import _native as nv
    from banzai_amd import corpus

    dev = torch.device("cuda", 0)

    def timed(fn):
        ts = []
        for _ in range(REPS):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t)
        return min(ts)

    row = {"step": step, "experiment": os.environ.get("BZH_RANGES_WIN", "")}
    with nv.Context(0, LEVEL, 0) as ctx:
        text = corpus.workload(N)[0].tobytes()
        d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).to(dev)
        cap = len(text) + len(text) // 4 + (1 << 20)
        d_comp = torch.zeros(cap, dtype=torch.uint8, device=dev)
        interval = 256 if step == "sync" else 0
        max_ent, max_pts = nv.encode_index_bound(LEVEL, len(text), interval)
        n, idx, pts = ctx.encode_index_device(d_text.data_ptr(), len(text), d_comp.data_ptr(), cap, interval, max_ent, max_pts)
        del d_text
        rng = random.Random(20261019)
        if step == "pieces":  # inside one block in the middle
            e = idx[len(idx) // 2]
            ranges = [(int(e["out_off"]) + rng.randrange(int(e["out_len"]) - SMALL_READ), SMALL_READ) for _ in range(SMALL)]
        else:
            ranges = [(rng.randrange(len(text) - READ), READ) for _ in range(READS)]
        want = text if step == "decode" else b"".join(text[o:o + ln] for o, ln in ranges)
        d_out = torch.zeros(len(want) + 64, dtype=torch.uint8, device=dev)
        row.update(stream_bytes=n, blocks=len(idx), reads=len(ranges), read_bytes=ranges[0][1], sync_points=len(pts))
        if step == "decode":
            def run(k=None):
                got, used = ctx.decode_device(d_comp.data_ptr(), n, d_out.data_ptr(), len(text))
                assert got == len(text) and used == n
        elif step == "loop":
            def run(k=len(ranges)):
                at = 0
                for off, ln in ranges[:k]:
                    at += ctx.decode_range_device(d_comp.data_ptr(), n, idx, off, ln, d_out.data_ptr() + at, ln)
        else:
            def run(k=None):
                st, total, _, _ = ctx.decode_ranges_device(d_comp.data_ptr(), n, idx, ranges, d_out.data_ptr(), len(want),
                                                           points=pts if step == "sync" else None)
                assert st == 0 and total == len(want), (st, total, ctx.last_error())
        run(1)  # warm-up: code objects, the arena (the loop: one read of it)
        d_out.zero_()
        row["seconds"] = timed(run)
        row["identical"] = d_out[:len(want)].cpu().numpy().tobytes() == want
        row["ms_per_read"] = 1e3 * row["seconds"] / len(ranges)
        if step not in ("decode", "loop"):
            row["ranges_stats"] = ctx.decode_ranges_stats()
        ctx.set_profiling(True)
        run(1)
        row["stages_ms"] = {k: v for k, v in ctx.decode_stats().items() if k.startswith("ms_")}
        ctx.set_profiling(False)
    print("ROW " + json.dumps(row), flush=True)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    rows = []
    steps = [(s, {}) for s in STEPS]
    if os.environ.get("BZH_EXPERIMENTS_LIB"):
        steps.append(("pieces", {"BZH_RANGES_WIN": "1", "BZH_LIB": os.environ["BZH_EXPERIMENTS_LIB"]}))
    for step, extra in steps:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", step], capture_output=True, text=True, timeout=420,
                           env={**os.environ, **extra})
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("ROW ")]
        if p.returncode != 0 or not line:
            print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
            sys.exit(f"step {step}: exit status {p.returncode}")
        rows.append(json.loads(line[0][4:]))
        print(json.dumps(rows[-1]), flush=True)
        if not rows[-1]["identical"]:
            sys.exit(f"step {step}: the output differs")
    result = {"workload": f"{N} bytes of the headline text at level {LEVEL}; {READS} reads of {READ} bytes; {SMALL} of {SMALL_READ} in one block",
              "best_of": REPS, "rows": rows}
    if out_path:
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    by = {r["step"]: r["seconds"] for r in rows if not r["experiment"]}
    if not by["ranges"] < by["loop"]:
        sys.exit(f"ranges: {by['ranges']:.3f} s for {READS} reads in one call, the loop of single reads takes {by['loop']:.3f} s")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main()
