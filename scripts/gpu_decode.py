"""Decode rates on cuda:0 against libbz2 on the same host (separate from bench.py): python scripts/gpu_decode.py [out.json] [repeats].
Inputs, all at level 9: the 100 MB headline text, real text when $BZH_ENWIK8 names a file, 1,000 concatenated 900 kB streams,
a 1 MB single-block stream (the latency case: one wavefront does the entropy stage alone).  For each: decoded MB/s with input
and output resident in HBM (bzh_decode_device) and host to host (bzh_decode), best of `repeats` after a warm-up, the stage
times of bzh_decode_stats from one more run with profiling on, and bz2.decompress of the same stream, single thread, timed
here (libbz2: the yardstick, not the code under test).  Both sides must give the same bytes."""
import bz2
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from banzai_amd import _native as nv  # noqa: E402
from banzai_amd import corpus  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else "gpu_decode.json"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
dev = torch.device("cuda", 0)


def best(fn, n=None):
    ts = []
    for _ in range(n or reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return min(ts), r


def inputs(ctx):
    text, name = corpus.workload(100_000_000)
    text = text.tobytes()
    yield f"100 MB text ({name})", ctx.encode(text), text
    path = os.environ.get("BZH_ENWIK8")
    if path and os.path.exists(path) and name != "enwik8":
        real = open(path, "rb").read()[:100_000_000]
        yield "real text ($BZH_ENWIK8)", ctx.encode(real), real
    parts = [text[k * 90_000:k * 90_000 + 880_000] for k in range(1000)]  # (880,000 bytes: one level-9 block a stream)
    yield "1,000 x 900 kB streams", b"".join(ctx.encode_many(parts)), b"".join(parts)
    yield "1 MB, one block", ctx.encode(text[:880_000]), text[:880_000]


res = {"level": 9, "repeats": reps, "rows": []}
ok = True
with nv.Context(0, 9, 0) as ctx:
    ctx.decode(ctx.encode(corpus.workload(3_000_000)[0].tobytes()))  # warm-up: code objects, the arena
    for name, stream, data in inputs(ctx):
        n_in, n_out = len(stream), len(data)
        d_in = torch.frombuffer(bytearray(stream), dtype=torch.uint8).to(dev)
        d_out = torch.empty(n_out + 64, dtype=torch.uint8, device=dev)
        ctx.set_profiling(False)
        ctx.decode_device(d_in.data_ptr(), n_in, d_out.data_ptr(), d_out.numel())  # warm-up of this shape
        t_dev, (got_n, used) = best(lambda: ctx.decode_device(d_in.data_ptr(), n_in, d_out.data_ptr(), d_out.numel()))
        same_dev = got_n == n_out and used == n_in and d_out[:got_n].cpu().numpy().tobytes() == data
        t_host, got = best(lambda: ctx.decode(stream, size_hint=n_out))
        ctx.set_profiling(True)
        ctx.decode_device(d_in.data_ptr(), n_in, d_out.data_ptr(), d_out.numel())
        st = ctx.decode_stats()
        ctx.set_profiling(False)
        t_cpu, ref = best(lambda: bz2.decompress(stream), 1 if n_out > 50_000_000 else reps)
        row = {"input": name, "stream_bytes": n_in, "decoded_bytes": n_out, "identical": bool(same_dev and got == data and ref == data),
               "device_s": t_dev, "host_s": t_host, "libbz2_s": t_cpu, "device_MB_per_s": n_out / t_dev / 1e6,
               "host_MB_per_s": n_out / t_host / 1e6, "libbz2_MB_per_s": n_out / t_cpu / 1e6, "stats": st}
        res["rows"].append(row)
        ok = ok and row["identical"]
        print(f"{name}: device {row['device_MB_per_s']:.0f} MB/s ({t_dev * 1e3:.1f} ms), host {row['host_MB_per_s']:.0f} MB/s, "
              f"libbz2 {row['libbz2_MB_per_s']:.1f} MB/s; stages ms: scan {st['ms_scan']:.2f} entropy {st['ms_entropy']:.2f} "
              f"unbwt {st['ms_unbwt']:.2f} unrle {st['ms_unrle']:.2f} crc {st['ms_crc']:.2f} total {st['ms_total']:.2f}; "
              f"blocks {st['blocks']} streams {st['streams']} candidates {st['candidates']} identical={row['identical']}", flush=True)
        del d_in, d_out
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        with open(out, "w") as f:  # (after every row: a run that is cut short keeps what it measured)
            json.dump(res, f, indent=1)
head = res["rows"][0]
print("device-resident decode of the 100 MB text is", "FASTER" if head["device_s"] < head["libbz2_s"] else "NOT faster", "than bz2.decompress")
if not ok:
    sys.exit(1)
