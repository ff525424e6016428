"""The matched parts alone (bzh_match*) on cuda:0: python scripts/gpu_match.py [out.json]
The 100 MB level-9 headline text of scripts/gpu_grep.py, everything the device calls need resident in HBM, device events round
every call, a warm-up first, and the sides of a comparison ALTERNATED inside one run, REPS rounds; every row keeps all of its
times (ms) and their median.  Every result is compared with a host loop.  Every step is a child process under a time limit of
its own; the first that fails ends the script.
  text       bzh_match_device of a rare word, [0-9]{4}, [A-Za-z]+ (nearly every byte comes back) and 16 words as a set, each
             beside bzh_search_device of the same pattern in the same child -- the lower bound: the matches are strictly more
             work -- and beside decode, copy and a host loop (re.finditer; the patterns are such that leftmost-first is
             leftmost-longest) that produces the same answer
  worst      100 MB of raw bytes through the raw seam: one repeated byte searched for two of it (every tile open), and .*x on
             newline-free text (every start holds a match of the full span), each beside a sparse text of the same size
Writes the JSON."""
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, LEVEL, REPS = 100_000_000, 9, 5


def setup():
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from banzai_amd import _native as nv
    from banzai_amd import corpus
    return np, torch, nv, corpus.workload(N)[0].tobytes()


def device_ms(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def child_text():
    np, torch, nv, text = setup()
    import banzai_amd
    dev = torch.device("cuda", 0)
    rare = next(w for w in text[:100_000].split() if len(w) >= 5 and 2_000 <= text.count(w) <= 50_000)
    words = sorted({w for w in text[:200_000].split() if 4 <= len(w) <= 12 and w.isalpha()}, key=lambda w: (-len(w), w))[:16]
    rows = []
    with nv.Context(0, LEVEL, 0) as ctx:
        d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).to(dev)
        cap = len(text) + len(text) // 4 + (1 << 20)
        d_comp = torch.zeros(cap, dtype=torch.uint8, device=dev)
        n = ctx.encode_device(d_text.data_ptr(), len(text), d_comp.data_ptr(), cap)
        n = int(n[0] if isinstance(n, tuple) else n)
        del d_text
        comp = d_comp[:n].cpu().numpy().tobytes()
        d_out = torch.zeros(len(text) + 64, dtype=torch.uint8, device=dev)
        cases = (("rare word", lambda: rare, re.escape(rare)),
                 ("[0-9]{4}", lambda: nv.PatternSet(ctx, [b"[0-9]{4}"], regex=True), b"[0-9]{4}"),
                 ("[A-Za-z]+", lambda: nv.PatternSet(ctx, [b"[A-Za-z]+"], regex=True), b"[A-Za-z]+"),
                 ("16 words", lambda: nv.PatternSet(ctx, words), b"|".join(re.escape(w) for w in words)))  # (longest first: leftmost-first is leftmost-longest)
        for name, make, host_re in cases:
            what = make()
            host = re.compile(host_re)

            def host_loop():
                plain = banzai_amd.decompress(comp)
                return b"".join(m.group() for m in host.finditer(plain))
            want = host_loop()
            want_n = sum(1 for _ in host.finditer(text))
            match = lambda: ctx.match_device(d_comp.data_ptr(), n, what, d_out.data_ptr(), len(text), 0)
            search = lambda: ctx.search_device(d_comp.data_ptr(), n, what, limit=0)
            st, nm, total, _ = match()  # the warm-up, and the check
            ok = st == 0 and nm == want_n and total == len(want) and d_out[:total].cpu().numpy().tobytes() == want
            stats = ctx.match_stats()
            search()
            t_match, t_search, t_host = [], [], []
            for k in range(REPS):  # alternated
                t_search.append(device_ms(torch, search))
                t_match.append(device_ms(torch, match))
                if k < 2:
                    t = time.perf_counter()
                    host_loop()
                    t_host.append((time.perf_counter() - t) * 1e3)
            rows.append({"case": name, "identical": bool(ok), "matches": int(nm), "out_bytes": int(total), "search_hits": int(search()[1]),
                         "match_ms": t_match, "search_ms": t_search, "host_ms": t_host, "match_median_ms": statistics.median(t_match),
                         "search_median_ms": statistics.median(t_search), "host_median_ms": statistics.median(t_host),
                         "match_over_search": statistics.median(t_match) / statistics.median(t_search),
                         "host_over_match": statistics.median(t_host) / statistics.median(t_match), "stats": stats})
            if hasattr(what, "close"):
                what.close()
    print("ROW " + json.dumps(rows), flush=True)


def child_worst():
    np, torch, nv, _ = setup()
    dev = torch.device("cuda", 0)
    rows = []
    with nv.Context(0, LEVEL, 0) as ctx:
        d_out = torch.zeros(N + 64, dtype=torch.uint8, device=dev)
        sparse = torch.full((N,), ord("b"), dtype=torch.uint8, device=dev)
        sparse[::100_003] = ord("a")
        sparse[1::100_003] = ord("a")
        run_a = torch.full((N,), ord("a"), dtype=torch.uint8, device=dev)
        run_x = torch.full((N,), ord("x"), dtype=torch.uint8, device=dev)
        cases = (("aa in a run of a (every tile open)", run_a, lambda: b"aa", N // 2, N // 2 * 2),
                 ("aa in a sparse text", sparse, lambda: b"aa", (N + 100_002) // 100_003, 2 * ((N + 100_002) // 100_003)),
                 (".*x in a run of x", run_x, lambda: nv.PatternSet(ctx, [b".*x"], regex=True), (N + 255) // 256, N))
        for name, d_raw, make, want_n, want_bytes in cases:
            what = make()
            call = lambda: ctx.match_raw_device(d_raw.data_ptr(), N, what, d_out.data_ptr(), N, 0)
            st, nm, total, _ = call()
            ok = st == 0 and nm == want_n and total == want_bytes
            stats = ctx.match_stats()
            times = [device_ms(torch, call) for _ in range(REPS)]
            rows.append({"case": name, "identical": bool(ok), "matches": int(nm), "out_bytes": int(total), "ms": times,
                         "median_ms": statistics.median(times), "stats": stats})
            if hasattr(what, "close"):
                what.close()
    rows[0]["dense_over_sparse"] = rows[0]["median_ms"] / rows[1]["median_ms"]
    print("ROW " + json.dumps(rows), flush=True)


def run_child(step):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", step], capture_output=True, text=True, timeout=540)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("ROW ")]
    if p.returncode != 0 or not line:
        print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
        sys.exit(f"step {step}: exit status {p.returncode}")
    return json.loads(line[0][4:])


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    result = {"workload": f"{N} bytes of the headline text at level {LEVEL}; {N} raw bytes for the worst cases", "reps": REPS}
    for step in ("worst", "text"):
        result[step] = run_child(step)
        print(json.dumps(result[step]), flush=True)
        if out_path:
            with open(out_path, "w") as f:
                json.dump(result, f, indent=1)
                f.write("\n")
    if not all(r["identical"] for step in ("worst", "text") for r in result[step]):
        sys.exit("a result differs from the host's")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        {"text": child_text, "worst": child_worst}[sys.argv[2]]()
    else:
        main()
