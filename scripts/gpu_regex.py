"""Regular expressions on cuda:0, measured: python scripts/gpu_regex.py [out.json]   (default profiles/r26_gpu_regex.json)
Level 9, the 100 MB headline text of scripts/gpu_index.py, everything resident in HBM, the median of 5 runs after a warm-up.
Every expression is measured twice, with its table staged in LDS and with BZH_REGEX_NO_LDS, as a grep counting call and as a
search counting call over the decoded text:
  word : one literal word as a Regex, as a PatternSet of one and as a single pattern -- the matcher's overhead;
  exprs: [0-9]{4}, [A-Za-z]+ing, 16 words as one alternation beside the same 16 as a PatternSet;
  worst: .*x at span 256 over 16 MB of one byte value that is not x (every start walks 256 steps and finds nothing), and over the
         text;
  full : bzh_grep_patset_device for one expression end to end beside bzh_decode_device on the same context, and beside decode,
         copy to the host and a host re.finditer.
Every step is a child process under a time limit of its own (the parent never opens the GPU); the first step that fails ends
the script.  Nothing is gated."""
import json
import os
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
import gpu_patset as ps  # noqa: E402  (median, words)

STEPS = (("encode", 300), ("word", 300), ("exprs", 420), ("worst", 300), ("full", 420))  # (name, seconds)
NO_LDS = 4


def both_paths(nv, ctx, exprs, d, n, flags=0, span=0, runs=ps.RUNS):
    """the grep and the search counting calls for `exprs`, rows in LDS and in HBM"""
    row = {}
    for name, extra in (("lds", 0), ("hbm", NO_LDS)):
        with nv.PatternSet(ctx, exprs, flags=flags | extra, regex=True, max_span=span) as r:
            t_grep, (st, nrecs, total, _) = ps.median(lambda: ctx.grep_raw_device(d.data_ptr(), n, r, 0, 0, 0), runs)
            assert st == 0
            t_search, (_, nhits) = ps.median(lambda: ctx.search_raw_device(d.data_ptr(), n, r, None, 0), runs)
            row[name] = {"grep_s": t_grep, "search_count_s": t_search, "records": nrecs, "hits": nhits, "grep_gb_s": n / t_grep / 1e9,
                         "search_gb_s": n / t_search / 1e9, "info": r.info}
    if row["lds"]["info"]["in_lds"]:
        assert (row["lds"]["records"], row["lds"]["hits"]) == (row["hbm"]["records"], row["hbm"]["hits"]), "the two paths find the same"
        row["hbm_over_lds_grep"] = row["hbm"]["grep_s"] / row["lds"]["grep_s"]
        row["hbm_over_lds_search"] = row["hbm"]["search_count_s"] / row["lds"]["search_count_s"]
    return row


def on_device(data):
    import torch
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


def step_word(work):
    from banzai_amd import _native as nv
    data, _ = base.text()
    d = on_device(data)
    word = ps.words(data, 1)[0]
    with nv.Context(0, 9, 0) as ctx:
        res = {"bytes": len(data), "word": word.decode(), "regex": both_paths(nv, ctx, [re.escape(word)], d, len(data))}
        count = lambda what: ctx.grep_raw_device(d.data_ptr(), len(data), what, 0, 0, 0)
        with nv.PatternSet(ctx, [word]) as pset:
            t, r = ps.median(lambda: count(pset))
            res["patset"] = {"grep_s": t, "records": r[1]}
        t, r = ps.median(lambda: count(word))
        res["single"] = {"grep_s": t, "records": r[1]}
        assert res["single"]["records"] == res["patset"]["records"] == res["regex"]["lds"]["records"]
    return res


def step_exprs(work):
    from banzai_amd import _native as nv
    data, _ = base.text()
    d = on_device(data)
    words = ps.words(data, 16)
    with nv.Context(0, 9, 0) as ctx:
        res = {"bytes": len(data), "digits4": both_paths(nv, ctx, [b"[0-9]{4}"], d, len(data)),
               "ing": both_paths(nv, ctx, [b"[A-Za-z]+ing"], d, len(data)),
               "alt16": both_paths(nv, ctx, [b"|".join(re.escape(w) for w in words)], d, len(data))}
        with nv.PatternSet(ctx, words) as pset:
            t, r = ps.median(lambda: ctx.grep_raw_device(d.data_ptr(), len(data), pset, 0, 0, 0))
            res["patset16"] = {"grep_s": t, "records": r[1], "info": pset.info}
        assert res["patset16"]["records"] == res["alt16"]["hbm"]["records"]
    return res


def step_worst(work):
    import torch
    from banzai_amd import _native as nv
    n = 16 << 20
    d = torch.full((n,), ord("z"), dtype=torch.uint8, device="cuda")
    data, _ = base.text()
    t = on_device(data)
    with nv.Context(0, 9, 0) as ctx:
        return {"one_byte_value": dict(both_paths(nv, ctx, [b".*x"], d, n, runs=3), bytes=n),
                "text": dict(both_paths(nv, ctx, [b".*x"], t, len(data), runs=3), bytes=len(data))}


def step_full(work):
    import torch
    from banzai_amd import _native as nv
    stream = open(os.path.join(work, "stream.bz2"), "rb").read()
    data, _ = base.text()
    d_in, d_out = base.resident(stream, len(data))
    expr = b"[A-Za-z]+ing"
    with nv.Context(0, 9, 0) as ctx:
        t_dec, (got, used) = ps.median(lambda: ctx.decode_device(d_in.data_ptr(), len(stream), d_out.data_ptr(), d_out.numel()))
        assert got == len(data)
        with nv.PatternSet(ctx, [expr], regex=True) as r:
            t_grep, (st, nrecs, total, _) = ps.median(lambda: ctx.grep_device(d_in.data_ptr(), len(stream), r, 0, 0, 0))
            assert st == 0
            stats = ctx.grep_stats()

        def host():
            ctx.decode_device(d_in.data_ptr(), len(stream), d_out.data_ptr(), d_out.numel())
            raw = d_out[:len(data)].cpu().numpy().tobytes()
            return sum(1 for _ in re.finditer(expr, raw))
        t0 = time.perf_counter()
        matches = host()
        t_host = time.perf_counter() - t0
    return {"expr": expr.decode(), "decode_s": t_dec, "grep_regex_s": t_grep, "grep_over_decode": t_grep / t_dec, "records": nrecs, "bytes": total,
            "decode_copy_finditer_s": t_host, "finditer_matches": matches, "stats": stats}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r26_gpu_regex.json")
    res = {}
    with tempfile.TemporaryDirectory() as work:
        for name, limit in STEPS:
            part = os.path.join(work, name + ".json")
            rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, work, part]).returncode
            if rc != 0:
                print(f"gpu_regex: step '{name}' ended with status {rc}; nothing further is started", flush=True)
                sys.exit(1)
            res[name] = json.load(open(part))
            os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
            with open(out, "w") as f:  # (after every step: a run that is cut short keeps what it measured)
                json.dump(res, f, indent=1)
            print(f"gpu_regex: step '{name}' done", flush=True)
    w = res["word"]
    print(f"one word: regex {w['regex']['lds']['grep_s'] * 1e3:.2f} ms (rows in HBM {w['regex']['hbm']['grep_s'] * 1e3:.2f} ms), "
          f"set of one {w['patset']['grep_s'] * 1e3:.2f} ms, single pattern {w['single']['grep_s'] * 1e3:.2f} ms")
    for k in ("digits4", "ing", "alt16"):
        r = res["exprs"][k]
        print(f"{k:8s}: grep lds {r['lds']['grep_s'] * 1e3:8.2f} ms, hbm {r['hbm']['grep_s'] * 1e3:8.2f} ms; search lds {r['lds']['search_count_s'] * 1e3:8.2f} ms, "
              f"hbm {r['hbm']['search_count_s'] * 1e3:8.2f} ms ({r['lds']['info']['states']} states x {r['lds']['info']['classes']} classes)")
    print(f"16 words as a set: {res['exprs']['patset16']['grep_s'] * 1e3:.2f} ms")
    for k in ("one_byte_value", "text"):
        r = res["worst"][k]
        print(f".*x over {k} ({r['bytes']} bytes): grep lds {r['lds']['grep_s'] * 1e3:.1f} ms, hbm {r['hbm']['grep_s'] * 1e3:.1f} ms")
    f = res["full"]
    print(f"grep of {f['expr']} end to end {f['grep_regex_s'] * 1e3:.1f} ms beside a decode of {f['decode_s'] * 1e3:.1f} ms and decode, copy, "
          f"re.finditer of {f['decode_copy_finditer_s'] * 1e3:.0f} ms")


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "--step":
        steps = {"encode": base.step_encode, "word": step_word, "exprs": step_exprs, "worst": step_worst, "full": step_full}
        json.dump(steps[sys.argv[2]](sys.argv[3]), open(sys.argv[4], "w"))
    else:
        main()
