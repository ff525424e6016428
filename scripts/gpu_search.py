"""Search inside a .bz2 on cuda:0: python scripts/gpu_search.py [out.json]
Everything resident in HBM, best of 3 after a warm-up, every step a child process under a time limit of its own; the first that
fails ends the script.  Every result is compared with the host's (a bytes.find loop over the text, the newlines in front of every
hit).  The input is the 100 MB level-9 headline text; the pattern is a word of it with thousands of hits, the delimiter the newline.
  decode      (a) bzh_decode_device -- existing code, the yardstick of `search`
  search      (b) bzh_search_device with record numbers: the same chain, every batch expanded into staging and searched there
  today       (c) what a user does without it: (a), the copy of the output to the host, a find loop there
  range       (d) bzh_decode_range_sync_device of the whole output at interval 256 -- existing code, the yardstick of `srange`
  srange      (e) bzh_search_range_device of the whole output with the same points and the record table
  raw         (f) bzh_search_raw_device on the raw text: both passes, the uploads and the wait -- NOT the kernel's rate
The script fails if `search` exceeds `decode`, or `srange` exceeds `range`, by more than the spread of the yardstick's own three runs
plus 1 ms (the added passes are memory-speed sweeps beside a serial walk), or if `search` is not below `today`.  Writes the JSON."""
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, LEVEL, REPS, INTERVAL = 100_000_000, 9, 3, 256
STEPS = ("decode", "search", "today", "range", "srange", "raw")


def find_all(text, pat):
    out, at = [], text.find(pat)
    while at >= 0:
        out.append(at)
        at = text.find(pat, at + 1)
    return out


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
        d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).to(dev)
        cap = len(text) + len(text) // 4 + (1 << 20)
        d_comp = torch.zeros(cap, dtype=torch.uint8, device=dev)
        max_ent, max_pts = nv.encode_index_bound(LEVEL, len(text), INTERVAL)
        n, idx, pts = ctx.encode_index_device(d_text.data_ptr(), len(text), d_comp.data_ptr(), cap, INTERVAL, max_ent, max_pts)
        # the pattern: the first word of five bytes or more that the text holds 2,000 to 50,000 times
        pat = next(w for w in text[:100_000].split() if len(w) >= 5 and 2_000 <= text.count(w) <= 50_000)
        want = find_all(text, pat)
        pos = np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == 10)
        want_rec = np.searchsorted(pos, np.array(want, dtype=np.int64)).tolist()
        ends = idx["out_off"] + idx["out_len"].astype(np.uint64)
        cum = np.concatenate([np.zeros(1, np.uint64), np.searchsorted(pos, ends.astype(np.int64)).astype(np.uint64)])
        row.update(stream_bytes=n, blocks=len(idx), sync_points=len(pts), pattern=pat.decode("latin-1"), hits=len(want))
        res = {}
        d_out = torch.zeros(len(text) + 64, dtype=torch.uint8, device=dev) if step in ("decode", "today", "range") else None
        got = ctypes.c_size_t(0)

        def hits_ok(r):
            hits, nhits = r
            return nhits == len(want) and hits["off"].tolist() == want and hits["record"].tolist() == want_rec

        if step == "decode":
            def run():
                res["ok"] = ctx.decode_device(d_comp.data_ptr(), n, d_out.data_ptr(), len(text)) == (len(text), n)
        elif step == "search":
            def run():
                res["ok"] = hits_ok(ctx.search_device(d_comp.data_ptr(), n, pat, delim=10, limit=len(want) + 16))
        elif step == "today":
            def run():
                total, used = ctx.decode_device(d_comp.data_ptr(), n, d_out.data_ptr(), len(text))
                host = d_out[:total].cpu().numpy().tobytes()
                res["ok"] = find_all(host, pat) == want
        elif step == "range":
            def run():
                ctx.check(nv.lib().bzh_decode_range_sync_device(ctx.handle, ctypes.c_void_p(d_comp.data_ptr()), n, 0, idx.ctypes.data_as(nv.idxp),
                                                                len(idx), pts.ctypes.data_as(nv.syncp), len(pts), 0, len(text),
                                                                ctypes.c_void_p(d_out.data_ptr()), len(text), ctypes.byref(got)))
                res["ok"] = got.value == len(text)
        elif step == "srange":
            def run():
                res["ok"] = hits_ok(ctx.search_range(n, idx, pat, 0, len(text), points=pts, rec_cum=cum, delim=10, limit=len(want) + 16,
                                                     d_in=d_comp.data_ptr()))
        else:
            def run():
                res["ok"] = hits_ok(ctx.search_raw_device(d_text.data_ptr(), len(text), pat, delim=10, limit=len(want) + 16))
        run()  # warm-up: code objects, the arena, the workspaces, the staging
        if step in ("decode", "range"):
            res["ok"] = res["ok"] and d_out[:len(text)].cpu().numpy().tobytes() == text
        ok = bool(res.get("ok"))
        ts = timed(run)
        row.update(seconds=min(ts), runs=ts, identical=ok and bool(res.get("ok")))
        if step in ("search", "srange", "raw"):
            row["search_stats"] = ctx.search_stats()
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
    result = {"workload": f"{N} bytes of the headline text at level {LEVEL}, sync points at interval {INTERVAL}; one word, records by newline",
              "best_of": REPS, "rows": rows}
    if out_path:
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    by = {r["step"]: r for r in rows}
    for new, old in (("search", "decode"), ("srange", "range")):
        spread = max(by[old]["runs"]) - min(by[old]["runs"])
        if by[new]["seconds"] > by[old]["seconds"] + spread + 1e-3:
            sys.exit(f"{new}: {by[new]['seconds']:.4f} s, {old} alone {by[old]['seconds']:.4f} s (spread {spread:.4f} s)")
    if not by["search"]["seconds"] < by["today"]["seconds"]:
        sys.exit(f"search: {by['search']['seconds']:.4f} s on the device, decode, copy and a host search {by['today']['seconds']:.4f} s")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main()
