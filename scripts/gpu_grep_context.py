"""Context records for the device grep on cuda:0: python scripts/gpu_grep_context.py [out.json] [--parent-lib libbzhip.so]
The 100 MB level-9 headline text of scripts/gpu_grep.py, everything the device calls need resident in HBM, device events round
every call, a warm-up first, and the sides of a comparison ALTERNATED inside one run, REPS rounds; every row keeps all of its
times (ms) and their median.  Every result is compared with a host split-find-dilate.  Every step is a child process under a time
limit of its own; the first that fails ends the script.
  parity     context 0, 0: bzh_grep_device of a rare word and of the regex [A-Za-z]+ing, this build against the library given with
             --parent-lib (the parent commit's build), children alternated.  The same kernels: the difference is to lie within
             the spread of one side's repeats.  Without --parent-lib the row says "not measured".
  price      -C 3 and -C 100 on the rare word and -C 3 on a letter that is on most lines, each beside the plain grep of the same
             pattern in the same child
  alternative  the same -C 3 result end to end from host bytes, banzai_amd.grep(context=3), against what a user does today:
             (a) decompress, and a split-and-dilate on the host; (b) grep followed by readv_records over a record index
Writes the JSON."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, LEVEL, REPS = 100_000_000, 9, 5
REGEX = b"[A-Za-z]+ing"


def setup():
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from banzai_amd import _native as nv
    from banzai_amd import corpus
    text = corpus.workload(N)[0].tobytes()
    rare = next(w for w in text[:100_000].split() if len(w) >= 5 and 2_000 <= text.count(w) <= 50_000)
    return np, torch, nv, text, rare


def truth(np, text, hit_records, before, after, invert=False):
    """-> (the selected records' numbers, their bytes' length, context records, groups) by split-find-dilate"""
    arr = np.frombuffer(text, dtype=np.uint8)
    pos = np.flatnonzero(arr == 10)
    ends = np.concatenate([pos + 1, [len(text)]]) if len(text) and text[-1] != 10 else pos + 1
    lens = np.diff(np.concatenate([[0], ends]))
    prim = np.zeros(len(ends), dtype=bool)
    prim[hit_records] = True
    if invert:
        prim = ~prim
    edge = np.zeros(len(ends) + 1, dtype=np.int64)
    p = np.flatnonzero(prim)
    np.add.at(edge, np.maximum(p - before, 0), 1)
    np.add.at(edge, np.minimum(p + after + 1, len(ends)), -1)
    sel = np.cumsum(edge[:-1]) > 0
    groups = int(np.count_nonzero(sel & ~np.concatenate([[False], sel[:-1]])))
    return np.flatnonzero(sel), int(lens[sel].sum()), int(np.count_nonzero(sel & ~prim)), groups, pos


def records_of_hits(np, text, pat, pos):
    found, at = [], text.find(pat)
    while at >= 0:
        found.append(at)
        at = text.find(pat, at + 1)
    return np.unique(np.searchsorted(pos, np.array(found, dtype=np.int64)))


def device_ms(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def encode(np, torch, nv, ctx, text):
    dev = torch.device("cuda", 0)
    d_text = torch.frombuffer(bytearray(text), dtype=torch.uint8).to(dev)
    cap = len(text) + len(text) // 4 + (1 << 20)
    d_comp = torch.zeros(cap, dtype=torch.uint8, device=dev)
    n = ctx.encode_device(d_text.data_ptr(), len(text), d_comp.data_ptr(), cap)
    del d_text
    return d_comp, int(n[0] if isinstance(n, tuple) else n)


def child_parity():
    """context 0, 0 with whatever library BZH_LIB names"""
    import re
    np, torch, nv, text, rare = setup()
    rows = {}
    with nv.Context(0, LEVEL, 0) as ctx:
        d_comp, n = encode(np, torch, nv, ctx, text)
        d_out = torch.zeros(len(text) + 64, dtype=torch.uint8, device=torch.device("cuda", 0))
        with nv.PatternSet(ctx, [REGEX], regex=True) as rx:
            for name, pat in (("rare", rare), ("regex", rx)):
                want = len([1 for ln in text.split(b"\n") if (rare in ln if name == "rare" else re.search(REGEX, ln))])
                call = lambda: ctx.grep_device(d_comp.data_ptr(), n, pat, d_out.data_ptr(), len(text), 0)
                st, nrecs, total, _ = call()  # the warm-up
                assert st == 0 and nrecs == want, (name, st, nrecs, want)
                rows[name] = [device_ms(torch, call) for _ in range(REPS)]
    print("ROW " + json.dumps(rows), flush=True)


def child_price():
    np, torch, nv, text, rare = setup()
    rows = []
    with nv.Context(0, LEVEL, 0) as ctx:
        d_comp, n = encode(np, torch, nv, ctx, text)
        d_out = torch.zeros(len(text) + 64, dtype=torch.uint8, device=torch.device("cuda", 0))
        pos = np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == 10)
        for name, pat, reach in (("rare -C 3", rare, 3), ("rare -C 100", rare, 100), ("common -C 3", b"e", 3)):
            hits = records_of_hits(np, text, pat, pos) if len(pat) > 1 else np.unique(np.searchsorted(pos, np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == pat[0])))
            want_rec, want_len, want_ctx, want_groups, _ = truth(np, text, hits, reach, reach)
            room = len(want_rec) + 16

            def run(b, a):
                ctx.grep_set_context(b, a)
                try:
                    return ctx.grep_device(d_comp.data_ptr(), n, pat, d_out.data_ptr(), len(text), room)
                finally:
                    ctx.grep_set_context(0, 0)
            st, nrecs, total, ent = run(reach, reach)  # the warm-up, and the check
            cs = ctx.grep_context_stats()
            ok = (st == 0 and nrecs == len(want_rec) and total == want_len and np.array_equal(ent["record"], want_rec)
                  and cs["context"] == want_ctx and cs["groups"] == want_groups and cs["matched"] == len(hits))
            run(0, 0)
            plain, with_ctx = [], []
            for _ in range(REPS):  # alternated
                plain.append(device_ms(torch, lambda: run(0, 0)))
                with_ctx.append(device_ms(torch, lambda: run(reach, reach)))
            rows.append({"case": name, "pattern": pat.decode("latin-1"), "identical": bool(ok), "matched": int(len(hits)), "selected": int(len(want_rec)),
                         "out_bytes": want_len, "groups": want_groups, "plain_ms": plain, "context_ms": with_ctx, "plain_median_ms": statistics.median(plain),
                         "context_median_ms": statistics.median(with_ctx), "ratio": statistics.median(with_ctx) / statistics.median(plain),
                         "context_stats": cs, "grep_stats": ctx.grep_stats()})
    print("ROW " + json.dumps(rows), flush=True)


def child_alternative():
    np, torch, nv, text, rare = setup()
    import banzai_amd
    with nv.Context(0, LEVEL, 0) as ctx:
        comp = ctx.encode(text)
    rindex = banzai_amd.build_record_index(comp)
    rd = banzai_amd.IndexedReader(comp, rindex)

    def with_context():
        return banzai_amd.grep(comp, rare, context=3)[0]

    def host_dilate():
        cut = banzai_amd.decompress(comp).split(b"\n")
        keep, last = [], len(cut) - 1
        for k, ln in enumerate(cut):
            if rare in ln:
                keep.extend(range(max(k - 3, keep[-1] + 1 if keep else 0), min(k + 3, last) + 1))
        return b"".join(cut[k] + b"\n" if k < last else cut[k] for k in keep)

    def grep_then_records():
        recs = banzai_amd.grep(comp, rare)[1]["record"].tolist()
        keep, last = [], rindex.nrecords - 1
        for r in recs:
            keep.extend(range(max(r - 3, keep[-1] + 1 if keep else 0), min(r + 3, last) + 1))
        runs, at = [], 0
        while at < len(keep):  # maximal runs of consecutive records: one (first, count) pair each
            end = at
            while end + 1 < len(keep) and keep[end + 1] == keep[end] + 1:
                end += 1
            runs.append((keep[at], end - at + 1))
            at = end + 1
        return b"".join(rd.readv_records(runs))

    sides = (("grep(context=3)", with_context), ("decompress, host split-and-dilate", host_dilate), ("grep, then readv_records", grep_then_records))
    first = [fn() for _, fn in sides]  # the warm-up, and the check
    ok = first[0] == first[1] == first[2] and len(first[0]) > 0
    times = {name: [] for name, _ in sides}
    for _ in range(REPS):  # alternated
        for name, fn in sides:
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t) * 1e3)
    med = {k: statistics.median(v) for k, v in times.items()}
    row = {"identical": bool(ok), "out_bytes": len(first[0]), "wall_ms": times, "median_ms": med,
           "host_dilate_over_context": med[sides[1][0]] / med[sides[0][0]], "grep_then_records_over_context": med[sides[2][0]] / med[sides[0][0]]}
    print("ROW " + json.dumps(row), flush=True)


def run_child(step, env=None):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", step], capture_output=True, text=True, timeout=540, env=env)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("ROW ")]
    if p.returncode != 0 or not line:
        print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
        sys.exit(f"step {step}: exit status {p.returncode}")
    return json.loads(line[0][4:])


def main():
    args = sys.argv[1:]
    parent = None
    if "--parent-lib" in args:
        at = args.index("--parent-lib")
        parent = os.path.abspath(args[at + 1])
        del args[at:at + 2]
    out_path = args[0] if args else None
    result = {"workload": f"{N} bytes of the headline text at level {LEVEL}; records by newline", "reps": REPS}
    if parent:
        sides = {"this": [], "parent": []}
        for _ in range(2):  # children alternated: this, parent, this, parent
            for side in ("this", "parent"):
                sides[side].append(run_child("parity", dict(os.environ, BZH_LIB=parent) if side == "parent" else None))
                print(side, json.dumps(sides[side][-1]), flush=True)
        parity = {}
        for name in ("rare", "regex"):
            a = [t for r in sides["this"] for t in r[name]]
            b = [t for r in sides["parent"] for t in r[name]]
            parity[name] = {"this_ms": a, "parent_ms": b, "this_median_ms": statistics.median(a), "parent_median_ms": statistics.median(b),
                            "this_spread_ms": max(a) - min(a), "parent_spread_ms": max(b) - min(b),
                            "difference_ms": statistics.median(a) - statistics.median(b)}
        result["parity"] = parity
    else:
        result["parity"] = "not measured"
    result["price"] = run_child("price")
    print(json.dumps(result["price"]), flush=True)
    result["alternative"] = run_child("alternative")
    print(json.dumps(result["alternative"]), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    if not all(r["identical"] for r in result["price"]) or not result["alternative"]["identical"]:
        sys.exit("a result differs from the host's")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        {"parity": child_parity, "price": child_price, "alternative": child_alternative}[sys.argv[2]]()
    else:
        main()
