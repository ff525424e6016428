"""The record table and reads by record number on cuda:0: python scripts/gpu_records.py [out.json]
Everything resident in HBM, best of 3 after a warm-up, every step a child process under a time limit of its own; the first that
fails ends the script.  Every step compares what it made byte for byte.  The input is the 100 MB level-9 headline text; the
delimiter is the newline.
  index     bzh_decode_index_sync_device at interval 256 -- existing code, the yardstick of `records`
  records   bzh_decode_index_records_device at interval 256: the same walk that also counts (unrle_count beside unrle_crc)
  raw       bzh_count_records_device on the raw text: the same table at memory bandwidth
  lines     256 seeded single-line reads in one bzh_decode_records_device call, with points
  today     the same lines as they must be fetched without this: bzh_decode_ranges_device of the whole touched blocks (it is even
            handed the table to know which), the blocks copied to the host, a search there -- the yardstick of `lines`
The script fails if `records` exceeds `index` by more than the spread of `index`'s own three runs plus 1 ms, or if `lines` is
slower than `today`: both are comparisons against existing code on the same box.  Writes the JSON."""
import ctypes
import json
import os
import random
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, LEVEL, REPS, INTERVAL, READS = 100_000_000, 9, 3, 256, 256
STEPS = ("index", "records", "raw", "lines", "today")


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
        arr = np.frombuffer(text, dtype=np.uint8)
        pos = np.flatnonzero(arr == 10)  # the newlines
        ends = idx["out_off"] + idx["out_len"].astype(np.uint64)
        want_cum = np.concatenate([np.zeros(1, np.uint64), np.searchsorted(pos, ends.astype(np.int64)).astype(np.uint64)])
        nrecords = len(pos) + (not text.endswith(b"\n"))
        row.update(stream_bytes=n, blocks=len(idx), sync_points=len(pts), delimiters=len(pos))
        res = {}
        if step == "index":
            ent = np.empty(max_ent, dtype=nv.INDEX_DTYPE)
            pp = np.empty(max(max_pts, 1), dtype=nv.SYNC_DTYPE)
            cnt, npts, used, total = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_uint64(0)

            def run():
                ctx.check(nv.lib().bzh_decode_index_sync_device(ctx.handle, ctypes.c_void_p(d_comp.data_ptr()), n, INTERVAL,
                                                                ent.ctypes.data_as(nv.idxp), max_ent, ctypes.byref(cnt),
                                                                pp.ctypes.data_as(nv.syncp), max_pts, ctypes.byref(npts), ctypes.byref(total),
                                                                ctypes.byref(used)))
                res["ok"] = ent[:cnt.value].tobytes() == idx.tobytes() and pp[:npts.value].tobytes() == pts.tobytes()
        elif step == "records":
            def run():
                e, p, cum, nrec, total, used = ctx.decode_index_records_device(d_comp.data_ptr(), n, INTERVAL, 10, max_ent, max_pts)
                res["ok"] = (e.tobytes() == idx.tobytes() and p.tobytes() == pts.tobytes() and cum.tolist() == want_cum.tolist()
                             and nrec == nrecords)
        elif step == "raw":
            def run():
                cum, nrec = ctx.count_records_device(d_text.data_ptr(), len(text), idx, 10)
                res["ok"] = cum.tolist() == want_cum.tolist() and nrec == nrecords
        else:
            rng = random.Random(20261019)
            lines = sorted(rng.sample(range(1, len(pos)), READS))
            want = [text[pos[r - 1] + 1:pos[r] + 1] for r in lines]
            ranges = [(r, 1) for r in lines]
            touched, _, _ = nv.record_spans(idx, want_cum, ranges)
            row.update(reads=READS, blocks_touched=len(touched), read_bytes=sum(len(w) for w in want))
            if step == "lines":
                d_out = torch.zeros(sum(len(w) for w in want) + 64, dtype=torch.uint8, device=dev)

                def run():
                    st, total, offs, lens = ctx.decode_records_device(d_comp.data_ptr(), n, idx, want_cum, ranges, d_out.data_ptr(),
                                                                      d_out.numel() - 64, points=pts)
                    assert st == 0, ctx.last_error()
                    host = d_out[:total].cpu().numpy().tobytes()
                    res["ok"] = [host[o:o + ln] for o, ln in zip(offs, lens)] == want
            else:
                blocks = [(int(idx[t]["out_off"]), int(idx[t]["out_len"])) for t in touched]
                d_out = torch.zeros(sum(ln for _, ln in blocks) + 64, dtype=torch.uint8, device=dev)

                def run():
                    st, total, offs, lens = ctx.decode_ranges_device(d_comp.data_ptr(), n, idx, blocks, d_out.data_ptr(), d_out.numel() - 64,
                                                                     points=pts)
                    assert st == 0, ctx.last_error()
                    host = d_out[:total].cpu().numpy()
                    got, at = [], {int(t): (o, ln) for t, o, ln in zip(touched, offs, lens)}
                    nl = {}
                    for r in lines:  # the line starts behind newline r and ends with newline r + 1, each in a touched block
                        ends_ = []
                        for k in (r, r + 1):
                            t = int(np.searchsorted(want_cum, k, side="left")) - 1
                            if t not in nl:
                                nl[t] = np.flatnonzero(host[at[t][0]:at[t][0] + at[t][1]] == 10)
                            ends_.append((t, int(nl[t][k - int(want_cum[t]) - 1]) + 1))
                        (t0, a), (t1, b) = ends_
                        if t0 == t1:
                            got.append(host[at[t0][0] + a:at[t0][0] + b].tobytes())
                        else:  # (adjacent touched blocks lie back to back in the output)
                            got.append(host[at[t0][0] + a:at[t1][0] + b].tobytes())
                    res["ok"] = got == want
        run()  # warm-up: code objects, the arena, the workspaces
        ts = timed(run)
        row.update(seconds=min(ts), runs=ts, identical=bool(res.get("ok")))
        if step in ("lines", "today"):
            row["ranges_stats"] = ctx.decode_ranges_stats()
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
    result = {"workload": f"{N} bytes of the headline text at level {LEVEL}, sync points at interval {INTERVAL}; {READS} single-line reads",
              "best_of": REPS, "rows": rows}
    if out_path:
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    by = {r["step"]: r for r in rows}
    spread = max(by["index"]["runs"]) - min(by["index"]["runs"])
    if by["records"]["seconds"] > by["index"]["seconds"] + spread + 1e-3:
        sys.exit(f"records: {by['records']['seconds']:.4f} s, the index build alone {by['index']['seconds']:.4f} s (spread {spread:.4f} s)")
    if by["lines"]["seconds"] > by["today"]["seconds"]:
        sys.exit(f"lines: {by['lines']['seconds']:.4f} s in one call, whole blocks and a host search {by['today']['seconds']:.4f} s")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main()
