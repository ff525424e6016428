"""Anchors and word boundaries on cuda:0, measured: python scripts/gpu_regex_look.py [out.json] [--parent-lib libbzhip.so]
(default profiles/r28_gpu_regex_look.json).  Level 9, the 100 MB headline text of scripts/gpu_index.py, everything resident in HBM,
the median of 5 runs after a warm-up; a grep counting call and a search counting call over the decoded text.
  free  : the assertion-free expressions of profiles/r26_gpu_regex.json -- [0-9]{4}, [A-Za-z]+ing, .*x -- which take the kernel
          instantiations they took before the assertions came.  With --parent-lib (a library built from the parent commit) the
          step runs twice per build, alternating, each in a process of its own: both builds and the spread between two runs of
          the same build stand side by side.  The claim is "no change beyond that spread".
  look  : ^[0-9]{4}, [0-9]{4}$, \\berror\\b and error under the word wrap, each beside its assertion-free form in the same process:
          the ratio.  No ratio is fixed in advance.
  full  : bzh_grep_patset_device for ^[A-Z] end to end beside bzh_decode_device on the same context.
Every step is a child process under a time limit of its own (the parent never opens the GPU); the first step that fails ends
the script.  Nothing is gated."""
import ctypes
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import gpu_index as base  # noqa: E402  (text, resident, step_encode)
import gpu_patset as ps  # noqa: E402  (median)

FREE = (("digits4", b"[0-9]{4}", 5), ("ing", b"[A-Za-z]+ing", 5), ("dot_star_x", b".*x", 3))
LOOK = (("bol_digits4", b"^[0-9]{4}", b"[0-9]{4}", 1), ("digits4_eol", b"[0-9]{4}$", b"[0-9]{4}", 1), ("word_error", b"\\berror\\b", b"error", 1),
        ("error_under_w", b"error", b"error", 3))  # (name, the expression, its assertion-free form, the syntax word: 1 ASSERT, 3 with WORD)


def on_device(data):
    import torch
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


def plain_regex(nv, ctx, exprs):
    """bzh_regex_create alone, as every build has it (a parent library knows no other call) -> a PatternSet"""
    arr = (ctypes.c_char_p * len(exprs))(*exprs)
    lens = (ctypes.c_size_t * len(exprs))(*[len(e) for e in exprs])
    h = ctypes.c_void_p()
    ctx.check(nv.lib().bzh_regex_create(ctx.handle, arr, lens, len(exprs), 0, 0, ctypes.byref(h)))
    r = nv.PatternSet.__new__(nv.PatternSet)
    r._h, r._destroy, r.info = h, nv.lib().bzh_patset_destroy, {}
    return r


def timed(ctx, d, n, r, runs):
    t_grep, (st, nrecs, total, _) = ps.median(lambda: ctx.grep_raw_device(d.data_ptr(), n, r, 0, 0, 0), runs)
    assert st == 0
    t_search, (_, nhits) = ps.median(lambda: ctx.search_raw_device(d.data_ptr(), n, r, None, 0), runs)
    return {"grep_s": t_grep, "search_count_s": t_search, "records": nrecs, "hits": nhits}


def step_free(work):
    from banzai_amd import _native as nv
    data, _ = base.text()
    d = on_device(data)
    res = {"bytes": len(data), "lib": os.path.basename(nv.LIB_PATH)}
    with nv.Context(0, 9, 0) as ctx:
        for name, expr, runs in FREE:
            with plain_regex(nv, ctx, [expr]) as r:
                res[name] = timed(ctx, d, len(data), r, runs)
    return res


def step_look(work):
    from banzai_amd import _native as nv
    data, _ = base.text()
    d = on_device(data)
    res = {"bytes": len(data)}
    with nv.Context(0, 9, 0) as ctx:
        for name, expr, free, syntax in LOOK:
            with nv.PatternSet(ctx, [expr], regex=True, syntax=syntax) as r, nv.PatternSet(ctx, [free], regex=True) as f:
                a, b = timed(ctx, d, len(data), r, 5), timed(ctx, d, len(data), f, 5)
                assert r.info["look_behind"] or r.info["look_ahead"]
                res[name] = {"look": a, "free": b, "info": r.info, "grep_ratio": a["grep_s"] / b["grep_s"], "search_ratio": a["search_count_s"] / b["search_count_s"]}
    return res


def step_full(work):
    from banzai_amd import _native as nv
    stream = open(os.path.join(work, "stream.bz2"), "rb").read()
    data, _ = base.text()
    d_in, d_out = base.resident(stream, len(data))
    expr = b"^[A-Z]"
    with nv.Context(0, 9, 0) as ctx:
        t_dec, (got, used) = ps.median(lambda: ctx.decode_device(d_in.data_ptr(), len(stream), d_out.data_ptr(), d_out.numel()))
        assert got == len(data)
        with nv.PatternSet(ctx, [expr], regex=True, syntax=1) as r:
            t_grep, (st, nrecs, total, _) = ps.median(lambda: ctx.grep_device(d_in.data_ptr(), len(stream), r, 0, 0, 0))
            assert st == 0
            stats = ctx.grep_stats()
    return {"expr": expr.decode(), "decode_s": t_dec, "grep_regex_s": t_grep, "grep_over_decode": t_grep / t_dec, "records": nrecs, "bytes": total, "stats": stats}


def main():
    args = sys.argv[1:]
    parent = None
    if "--parent-lib" in args:
        at = args.index("--parent-lib")
        parent = os.path.abspath(args[at + 1])
        del args[at:at + 2]
    out = args[0] if args else os.path.join(ROOT, "profiles", "r28_gpu_regex_look.json")
    steps = [("encode", "encode", 300, None), ("free_a", "free", 300, None)]
    if parent:
        steps += [("free_parent_a", "free", 300, parent), ("free_b", "free", 300, None), ("free_parent_b", "free", 300, parent)]
    steps += [("look", "look", 420, None), ("full", "full", 420, None)]
    res = {}
    with tempfile.TemporaryDirectory() as work:
        for key, name, limit, lib in steps:
            part = os.path.join(work, key + ".json")
            env = dict(os.environ, BZH_LIB=lib) if lib else os.environ
            rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, work, part], env=env).returncode
            if rc != 0:
                print(f"gpu_regex_look: step '{key}' ended with status {rc}; nothing further is started", flush=True)
                sys.exit(1)
            res[key] = json.load(open(part))
            os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
            with open(out, "w") as f:  # (after every step: a run that is cut short keeps what it measured)
                json.dump(res, f, indent=1)
            print(f"gpu_regex_look: step '{key}' done", flush=True)
    for name, expr, _ in FREE:
        row = f"{expr.decode():14s}: grep " + ", ".join(f"{k} {res[k][name]['grep_s'] * 1e3:.3f} ms" for k, step, _, _ in steps if step == "free")
        print(row)
        if parent:
            this, old = [res[k][name]["grep_s"] for k in ("free_a", "free_b")], [res[k][name]["grep_s"] for k in ("free_parent_a", "free_parent_b")]
            res.setdefault("free_summary", {})[name] = {"this_over_parent": (sum(this) / 2) / (sum(old) / 2), "spread_this": max(this) / min(this),
                                                        "spread_parent": max(old) / min(old)}
    for name, expr, free, syntax in LOOK:
        r = res["look"][name]
        print(f"{expr.decode():14s} (syntax {syntax}): grep {r['look']['grep_s'] * 1e3:.3f} ms, {r['grep_ratio']:.2f} x {free.decode()}; "
              f"search {r['look']['search_count_s'] * 1e3:.3f} ms, {r['search_ratio']:.2f} x")
    f = res["full"]
    print(f"grep of {f['expr']} end to end {f['grep_regex_s'] * 1e3:.1f} ms beside a decode of {f['decode_s'] * 1e3:.1f} ms")
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "--step":
        fns = {"encode": base.step_encode, "free": step_free, "look": step_look, "full": step_full}
        json.dump(fns[sys.argv[2]](sys.argv[3]), open(sys.argv[4], "w"))
    else:
        main()
