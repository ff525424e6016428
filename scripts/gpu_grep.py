"""Grep inside a .bz2 on cuda:0: python scripts/gpu_grep.py [out.json]
Everything resident in HBM, best of 3 after a warm-up, every step a child process under a time limit of its own; the first that
fails ends the script.  Every result is compared with the host's: the text cut at its newlines, a record selected when a match
starts inside it.  The input is the 100 MB level-9 headline text of scripts/gpu_search.py; the rare needle is its word (thousands
of hits), the common one a single letter that is on nearly every line.
  decode        bzh_decode_device -- existing code
  search        bzh_search_device with the rare needle and record numbers -- existing code
  grep          bzh_grep_device with the rare needle: the lines and their entries
  grep_common   ... with the common needle: nearly every byte is copied
  grep_invert   ... with the rare needle inverted: nearly every byte is copied
  grep_index    bzh_grep_index_device with the rare needle and sync points at interval 256
  raw           bzh_grep_raw_device on the raw text, rare needle: the passes, the uploads and the wait -- NOT the kernel's rate
  today         what a user does without it: bzh_decode_device, the copy of the output to the host, a split-and-filter there
The script fails if a grep row is slower than `today` in the same run.  Writes the JSON."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, LEVEL, REPS, INTERVAL = 100_000_000, 9, 3, 256
STEPS = ("decode", "search", "grep", "grep_common", "grep_invert", "grep_index", "raw", "today")
GREPS = ("grep", "grep_common", "grep_invert", "grep_index", "raw")


def child(step):
    import numpy as np
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
        return ts

    row = {"step": step}
    with nv.Context(0, LEVEL, 0) as ctx:
        text = corpus.workload(N)[0].tobytes()
        arr = np.frombuffer(text, dtype=np.uint8)
        d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).to(dev)
        cap = len(text) + len(text) // 4 + (1 << 20)
        d_comp = torch.zeros(cap, dtype=torch.uint8, device=dev)
        max_ent, max_pts = nv.encode_index_bound(LEVEL, len(text), INTERVAL)
        n, idx, pts = ctx.encode_index_device(d_text.data_ptr(), len(text), d_comp.data_ptr(), cap, INTERVAL, max_ent, max_pts)
        rare = next(w for w in text[:100_000].split() if len(w) >= 5 and 2_000 <= text.count(w) <= 50_000)
        pat = b"e" if step == "grep_common" else rare
        invert = step == "grep_invert"
        # the truth: the records (the delimiter belongs to the record it ends), those in which a match starts
        pos = np.flatnonzero(arr == 10)
        ends = np.concatenate([pos + 1, [len(text)]]) if len(text) and text[-1] != 10 else pos + 1
        starts = np.concatenate([[0], ends[:-1]])
        if len(pat) == 1:
            hits = np.flatnonzero(arr == pat[0])
        else:
            found, at = [], text.find(pat)
            while at >= 0:
                found.append(at)
                at = text.find(pat, at + 1)
            hits = np.array(found, dtype=np.int64)
        sel = np.zeros(len(ends), dtype=bool)
        sel[np.searchsorted(pos, hits)] = True
        if invert:
            sel = ~sel
        lens = ends - starts
        want_rec = np.flatnonzero(sel)
        want = arr[np.repeat(sel, lens)].tobytes()
        want_len = lens[sel]
        want_out = np.concatenate([[0], np.cumsum(want_len)[:-1]]) if len(want_len) else want_len
        row.update(stream_bytes=n, blocks=len(idx), sync_points=len(pts), pattern=pat.decode("latin-1"), invert=invert,
                   records=int(len(ends)), selected=int(len(want_rec)), out_bytes=len(want), hits=int(len(hits)))
        res = {}
        d_out = torch.zeros(len(text) + 64, dtype=torch.uint8, device=dev)
        room = len(want_rec) + 16

        def grep_ok(r):
            st, nrecs, total, ent = r
            return (st == 0 and nrecs == len(want_rec) and total == len(want) and np.array_equal(ent["record"], want_rec)
                    and np.array_equal(ent["off"], starts[sel]) and np.array_equal(ent["len"], want_len) and np.array_equal(ent["out_off"], want_out))

        if step == "decode":
            def run():
                res["ok"] = ctx.decode_device(d_comp.data_ptr(), n, d_out.data_ptr(), len(text)) == (len(text), n)
        elif step == "search":
            def run():
                h, nh = ctx.search_device(d_comp.data_ptr(), n, pat, delim=10, limit=len(hits) + 16)
                res["ok"] = nh == len(hits) and np.array_equal(h["off"], hits)
        elif step == "today":
            def run():
                total, used = ctx.decode_device(d_comp.data_ptr(), n, d_out.data_ptr(), len(text))
                host = d_out[:total].cpu().numpy().tobytes()
                cut = host.split(b"\n")
                res["ok"] = b"".join(ln + b"\n" for ln in cut[:-1] if pat in ln) + (cut[-1] if pat in cut[-1] else b"") == want
        elif step == "grep_index":
            def run():
                res["ok"] = grep_ok(ctx.grep_index_device(d_comp.data_ptr(), n, idx, pat, d_out.data_ptr(), len(text), room, points=pts))
        elif step == "raw":
            def run():
                res["ok"] = grep_ok(ctx.grep_raw_device(d_text.data_ptr(), len(text), pat, d_out.data_ptr(), len(text), room))
        else:
            def run():
                res["ok"] = grep_ok(ctx.grep_device(d_comp.data_ptr(), n, pat, d_out.data_ptr(), len(text), room, invert=invert))
        run()  # warm-up: code objects, the arena, the workspaces, the staging
        if step == "decode":
            res["ok"] = res["ok"] and d_out[:len(text)].cpu().numpy().tobytes() == text
        if step in GREPS:
            res["ok"] = res["ok"] and d_out[:len(want)].cpu().numpy().tobytes() == want
        ok = bool(res.get("ok"))
        ts = timed(run)
        row.update(seconds=min(ts), runs=ts, identical=ok and bool(res.get("ok")))
        if step in GREPS:
            row["grep_stats"] = ctx.grep_stats()
    print("ROW " + json.dumps(row), flush=True)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    rows = []
    for step in STEPS:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", step], capture_output=True, text=True, timeout=420)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("ROW ")]
        if p.returncode != 0 or not line:
            print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
            sys.exit(f"step {step}: exit status {p.returncode}")
        rows.append(json.loads(line[0][4:]))
        print(json.dumps(rows[-1]), flush=True)
        if not rows[-1]["identical"]:
            sys.exit(f"step {step}: the result differs")
    result = {"workload": f"{N} bytes of the headline text at level {LEVEL}, sync points at interval {INTERVAL}; records by newline",
              "best_of": REPS, "rows": rows}
    if out_path:
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    by = {r["step"]: r for r in rows}
    for g in GREPS:
        if by[g]["seconds"] > by["today"]["seconds"]:
            sys.exit(f"{g}: {by[g]['seconds']:.4f} s on the device, decode, copy and a host split-and-filter {by['today']['seconds']:.4f} s")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main()
