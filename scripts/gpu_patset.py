"""A set of patterns in one pass on cuda:0, measured: python scripts/gpu_patset.py [out.json]   (default profiles/r25_gpu_patset.json)
Level 9, the 100 MB headline text of scripts/gpu_index.py, everything resident in HBM, the median of 5 runs after a warm-up:
  raw  : bzh_grep_patset_raw_device as a counting call over the decoded text for K in {1, 16, 256, 4096} distinct words drawn from
         the text, with and without BZH_PATSET_FOLD_ASCII, beside the baseline -- K successive bzh_grep_raw_device counting calls
         on the same resident bytes, what a user does today (for K = 4096 the first 64 are timed and the sum scaled);
  full : bzh_grep_patset_device (16 words, counting) end to end beside bzh_decode_device on the same context;
  worst: the adversarial text of one byte value, 16 MB, with the 256-byte pattern of that byte and all its shorter runs.
Every step is a child process under a time limit of its own (the parent never opens the GPU); the first step that fails ends
the script.  The one condition: at K = 16 the set pass takes less time than the 16 single-pattern passes."""
import json
import os
import random
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import gpu_index as base  # noqa: E402  (text, resident, step_encode)

STEPS = (("encode", 300), ("raw", 420), ("full", 300), ("worst", 300))  # (name, seconds)
KS = (1, 16, 256, 4096)
RUNS = 5


def median(fn, runs=RUNS):
    import torch
    fn()  # warm-up
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return statistics.median(ts), r


def words(data, k):
    """k distinct words of 3 to 12 letters drawn from the text, seeded"""
    seen = sorted(set(re.findall(rb"[A-Za-z]{3,12}", data[:8_000_000])))
    random.Random(k).shuffle(seen)
    assert len(seen) >= k, f"the text holds {len(seen)} distinct words"
    return seen[:k]


def step_raw(work):
    import torch
    from banzai_amd import _native as nv
    data, _ = base.text()
    d = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    res = {"bytes": len(data), "runs": RUNS, "k": {}}
    with nv.Context(0, 9, 0) as ctx:
        count = lambda what: ctx.grep_raw_device(d.data_ptr(), len(data), what, 0, 0, 0)
        for k in KS:
            pats = words(data, k)
            timed = pats[:64]
            singles = [median(lambda p=p: count(p)) for p in timed]
            assert all(r[0] == 0 for _, r in singles)
            baseline = sum(t for t, _ in singles) * (k / len(timed))
            row = {"baseline_s": baseline, "baseline_timed_calls": len(timed), "single_median_s": statistics.median(t for t, _ in singles)}
            for fold in (False, True):
                with nv.PatternSet(ctx, pats, fold) as pset:
                    t, (st, nrecs, total, _) = median(lambda: count(pset))
                    assert st == 0
                    if k == 1 and not fold:
                        assert (nrecs, total) == singles[0][1][1:3], "a set of one selects what the single pattern selects"
                    row["fold" if fold else "exact"] = {"set_s": t, "records": nrecs, "bytes": total, "info": pset.info, "baseline_over_set": baseline / t,
                                                        "stats": ctx.grep_stats()}
            res["k"][str(k)] = row
    return res


def step_full(work):
    from banzai_amd import _native as nv
    stream = open(os.path.join(work, "stream.bz2"), "rb").read()
    data, _ = base.text()
    d_in, d_out = base.resident(stream, len(data))
    with nv.Context(0, 9, 0) as ctx:
        t_dec, (got, used) = median(lambda: ctx.decode_device(d_in.data_ptr(), len(stream), d_out.data_ptr(), d_out.numel()))
        assert got == len(data)
        with nv.PatternSet(ctx, words(data, 16), True) as pset:
            t_set, (st, nrecs, total, _) = median(lambda: ctx.grep_device(d_in.data_ptr(), len(stream), pset, 0, 0, 0))
            assert st == 0
            stats = ctx.grep_stats()
    return {"decode_s": t_dec, "grep_patset_s": t_set, "grep_over_decode": t_set / t_dec, "records": nrecs, "bytes": total, "stats": stats}


def step_worst(work):
    import torch
    from banzai_amd import _native as nv
    n = 16 << 20
    d = torch.full((n,), ord("z"), dtype=torch.uint8, device="cuda")
    with nv.Context(0, 9, 0) as ctx:
        res = {"bytes": n}
        for name, pats in (("one_of_256", [b"z" * 256]), ("every_run_to_256", [b"z" * k for k in range(1, 257)])):
            with nv.PatternSet(ctx, pats) as pset:
                t_grep, (st, nrecs, _, _) = median(lambda: ctx.grep_raw_device(d.data_ptr(), n, pset, 0, 0, 0), 3)
                assert st == 0 and nrecs == 1
                t_search, (_, nhits) = median(lambda: ctx.search_raw_device(d.data_ptr(), n, pset, None, 0), 3)
                assert nhits == sum(n - len(p) + 1 for p in pats)
                res[name] = {"grep_s": t_grep, "search_count_s": t_search, "hits": nhits, "grep_gb_s": n / t_grep / 1e9, "search_gb_s": n / t_search / 1e9}
        t_one, _ = median(lambda: ctx.grep_raw_device(d.data_ptr(), n, b"z" * 256, 0, 0, 0), 3)
        res["single_pattern_grep_s"] = t_one
    return res


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r25_gpu_patset.json")
    res = {}
    with tempfile.TemporaryDirectory() as work:
        for name, limit in STEPS:
            part = os.path.join(work, name + ".json")
            rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, work, part]).returncode
            if rc != 0:
                print(f"gpu_patset: step '{name}' ended with status {rc}; nothing further is started", flush=True)
                sys.exit(1)
            res[name] = json.load(open(part))
            os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
            with open(out, "w") as f:  # (after every step: a run that is cut short keeps what it measured)
                json.dump(res, f, indent=1)
            print(f"gpu_patset: step '{name}' done", flush=True)
    for k in KS:
        r = res["raw"]["k"][str(k)]
        print(f"K {k:5d}: set {r['exact']['set_s'] * 1e3:8.2f} ms, folded {r['fold']['set_s'] * 1e3:8.2f} ms; {k} single passes {r['baseline_s'] * 1e3:9.2f} ms "
              f"({r['exact']['info']['states']} states, {r['exact']['info']['classes']} classes, {r['exact']['info']['table_bytes']} bytes)")
    f = res["full"]
    print(f"grep of 16 words end to end {f['grep_patset_s'] * 1e3:.1f} ms beside a decode of {f['decode_s'] * 1e3:.1f} ms")
    w = res["worst"]
    print(f"one byte value, {w['bytes']} bytes: grep {w['one_of_256']['grep_s'] * 1e3:.1f} ms, search of every run {w['every_run_to_256']['search_count_s'] * 1e3:.1f} ms")
    r16 = res["raw"]["k"]["16"]
    if not max(r16["exact"]["set_s"], r16["fold"]["set_s"]) < r16["baseline_s"]:
        print("gpu_patset: at K = 16 the set pass is NOT faster than the 16 single-pattern passes")
        sys.exit(1)


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "--step":
        steps = {"encode": base.step_encode, "raw": step_raw, "full": step_full, "worst": step_worst}
        json.dump(steps[sys.argv[2]](sys.argv[3]), open(sys.argv[4], "w"))
    else:
        main()
