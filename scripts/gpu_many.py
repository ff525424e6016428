"""encode_many against a loop of Context.encode over the same inputs, on cuda:0 (separate from bench.py).
Inputs: seeded slices of corpus.enwik_synthetic_v2 plus a random share; a warm-up first; both sides must give the same bytes.
Prints streams/s and MB/s for 4,096 x 4 KiB, 1,024 x 64 KiB and 256 x 1 MB (argv: [out.json] [repeats])."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from banzai_amd import _native as nv  # noqa: E402
from banzai_amd import corpus  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else "gpu_many.json"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
CONFIGS = [(4096, 4096), (1024, 65536), (256, 1_000_000)]
RANDOM_SHARE = 0.1


def inputs(count, size, seed):
    rng = np.random.default_rng(seed)
    text = corpus.enwik_synthetic_v2(min(count * size, 64 << 20) + size, seed=seed).tobytes()
    items = []
    for k in range(count):
        if rng.random() < RANDOM_SHARE:
            items.append(rng.integers(0, 256, size, dtype=np.uint8).tobytes())
        else:
            o = int(rng.integers(0, len(text) - size))
            items.append(text[o:o + size])
    return items


def best(fn):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        r = fn()
        ts.append(time.perf_counter() - t)
    return min(ts), r


res = {"level": 9, "repeats": reps, "random_share": RANDOM_SHARE, "configs": []}
with nv.Context(0, 9, 0) as ctx:
    warm = inputs(64, 4096, 1)
    ctx.encode_many(warm)
    [ctx.encode(x) for x in warm[:8]]
    for count, size in CONFIGS:
        items = inputs(count, size, count)
        mb = count * size / 1e6
        t_many, many = best(lambda: ctx.encode_many(items))
        t_loop, loop = best(lambda: [ctx.encode(x) for x in items])
        row = {"count": count, "size": size, "identical": many == loop,
               "many_s": t_many, "loop_s": t_loop,
               "many_streams_per_s": count / t_many, "loop_streams_per_s": count / t_loop,
               "many_MB_per_s": mb / t_many, "loop_MB_per_s": mb / t_loop, "speedup": t_loop / t_many,
               "out_bytes": sum(len(s) for s in many)}
        res["configs"].append(row)
        print(f"{count:5d} x {size:8d}: encode_many {row['many_streams_per_s']:10.0f} streams/s {row['many_MB_per_s']:8.1f} MB/s | "
              f"loop {row['loop_streams_per_s']:8.0f} streams/s {row['loop_MB_per_s']:8.1f} MB/s | x{row['speedup']:.1f} "
              f"identical={row['identical']}", flush=True)
os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
with open(out, "w") as f:
    json.dump(res, f, indent=1)
if not all(r["identical"] for r in res["configs"]):
    sys.exit(1)
