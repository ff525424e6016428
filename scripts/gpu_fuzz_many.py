"""On-box fuzz of bzh_encode_many, modelled on scripts/gpu_fuzz.py: random LISTS of inputs (empty ones, runs that go on across
neighbours, sizes around the block budget) at random levels, batch sizes and Huffman modes; every stream compared bit for bit
with the CPU oracle's (reference mode) or with bzh_encode of the input alone (fixed mode), and decoded again by libbz2.
Time-boxed, seeded, on cuda:0; writes a JSON summary (argv: seconds [seed] [out.json])."""
import bz2
import json
import os
import random
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from banzai_amd import _native as nv  # noqa: E402
from oracle import pyoracle as po  # noqa: E402
from tests import cases  # noqa: E402

seconds = float(sys.argv[1]) if len(sys.argv) > 1 else 120
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
out = sys.argv[3] if len(sys.argv) > 3 else "fuzz_many.json"
rng = random.Random(seed)
ctxs = {(lv, mb): nv.Context(0, lv, mb) for lv in (1, 2, 9) for mb in (3, 8, 0)}
t0 = time.time()
stats = {"seed": seed, "seconds": seconds, "lists": 0, "streams": 0, "bytes": 0, "fixed_lists": 0, "failures": []}


def item(rng, level):
    kind = rng.randrange(6)
    n = rng.choice([0, 0, 1, 3, 4, 5, 255, 256, 259, 4096, 30_000, 100_000 * level - 1, 100_000 * level + 300, 250_000])
    if kind == 0:
        return cases.mixture(rng, max(1, n))
    if kind == 1:  # one byte repeated: runs that a neighbour may continue
        return bytes([rng.randrange(3)]) * n
    if kind == 2:
        w = bytes(rng.randrange(256) for _ in range(rng.choice([1, 2, 7, 64])))
        return (w * (n // len(w) + 1))[:n]
    if kind == 3:
        return bytes(rng.randrange(256) for _ in range(min(n, 50_000)))
    return cases.gen(n, rng.choice(["text", "longruns", "shortruns", "same", "random", "periodic"]), rng.randrange(1 << 30))


while time.time() - t0 < seconds:
    lv = rng.choice([1, 2, 9])
    mb = rng.choice([3, 8, 0])
    fixed = rng.random() < 0.2
    items = [item(rng, lv) for _ in range(rng.choice([1, 2, 5, 17, 64, 300]))]
    ctx = ctxs[(lv, mb)]
    try:
        ctx.set_mode(fixed)
        got = ctx.encode_many(items)
        if fixed:
            ref = ctxs[(lv, 0)] if mb else ctxs[(lv, 8)]
            ref.set_mode(True)
            want = [ref.encode(x) for x in items]
            ref.set_mode(False)
        else:
            want = [po.encode(x, lv) for x in items]
        ok = got == want and all(bz2.decompress(g) == x for g, x in zip(got, items))
    except Exception as e:  # noqa: BLE001
        ok = False
        stats["failures"].append({"list": stats["lists"], "error": repr(e)})
    finally:
        ctx.set_mode(False)
    if not ok and (not stats["failures"] or stats["failures"][-1].get("list") != stats["lists"]):
        stats["failures"].append({"list": stats["lists"], "level": lv, "max_batch": mb, "fixed": fixed,
                                  "lens": [len(x) for x in items][:64]})
    stats["lists"] += 1
    stats["fixed_lists"] += fixed
    stats["streams"] += len(items)
    stats["bytes"] += sum(len(x) for x in items)
stats["elapsed"] = time.time() - t0
os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
with open(out, "w") as f:
    json.dump(stats, f, indent=1)
print(json.dumps({k: v for k, v in stats.items() if k != "failures"}), "failures:", len(stats["failures"]))
sys.exit(1 if stats["failures"] else 0)
