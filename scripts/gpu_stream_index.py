"""The streaming encoder's index on cuda:0, measured: python scripts/gpu_stream_index.py [out.json]   (default profiles/r19_gpu_stream_index.json)
Level 9, the 100 MB headline text of scripts/gpu_index.py, host buffers in and out through bzh_stream_feed in 16 MiB feeds (what
bnzhip and banzai_amd.encode do), best of 3 after a warm-up, the three variants taking turns inside every repeat:
  stream  : (a) bzh_stream_begin -- the parent's path, the yardstick; (b) bzh_stream_begin_index at interval 256 and (c) at
            interval 0, bzh_stream_index_take after every feed; the three streams are compared, and the taken arrays with
            bzh_encode_index's, byte for byte;
  oneshot : what the index would otherwise cost: (d) bzh_encode_index of the whole input, (e) bzh_decode_index_sync of the
            stream at interval 256, whose arrays are compared with the taken ones as well.
The script fails only if (b) is not below (a) + (e): an index recorded while streaming must be cheaper than streaming plainly and
building the index by a decode pass.  It prints the table of DESIGN.md section 7.  Every step is a child process under a time
limit of its own (the parent never opens the GPU); the first step that fails ends the script."""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import gpu_index as base  # noqa: E402  (text)

STEPS = (("stream", 420), ("oneshot", 420))  # (name, seconds)
FEED = 16 << 20
REPS = 3


def run_stream(ctx, view, interval):
    """one stream over `view` in FEED-byte feeds; interval None: no index -> (seconds, stream bytes, entries, points)"""
    import numpy as np
    from banzai_amd import _native as nv
    t = time.perf_counter()  # (every call below returns with its bytes in host memory: nothing is left running on the device)
    if interval is None:
        ctx.stream_begin()
    else:
        ctx.stream_begin_index(interval)
    out, ents, pts = [], [np.zeros(0, nv.INDEX_DTYPE)], [np.zeros(0, nv.SYNC_DTYPE)]
    pos, n = 0, len(view)
    while True:
        k = min(FEED, n - pos)
        got = ctx.stream_feed_view(view[pos:pos + k], k == 0)
        pos += k
        if len(got):
            out.append(bytes(got))
        if interval is not None:
            e, p = ctx.stream_index_take()
            ents.append(e)
            pts.append(p)
        if k == 0:
            break
    dt = time.perf_counter() - t
    return dt, b"".join(out), np.concatenate(ents), np.concatenate(pts)


def step_stream(work):
    from banzai_amd import _native as nv
    data, name = base.text()
    view = memoryview(data)
    res = {"input": f"100 MB text ({name})", "level": 9, "repeats": REPS, "feed_bytes": FEED}
    variants = (("plain", None), ("index_256", 256), ("index_0", 0))
    times = {k: [] for k, _ in variants}
    kept = {}
    with nv.Context(0, 9, 0) as ctx:
        for key, interval in variants:  # warm-up of every variant
            run_stream(ctx, view, interval)
        for _ in range(REPS):
            for key, interval in variants:
                dt, stream, ent, pts = run_stream(ctx, view, interval)
                times[key].append(dt)
                kept[key] = (stream, ent, pts)
        stream = kept["plain"][0]
        for key, interval in variants[1:]:
            s2, ent, pts = kept[key]
            assert s2 == stream, f"{key}: the stream differs from plain streaming's"
            s1, e1, p1 = ctx.encode_index(data, interval)
            assert s1 == stream and ent.tobytes() == e1.tobytes() and pts.tobytes() == p1.tobytes(), f"{key}: not bzh_encode_index's arrays"
            res[f"{key}_points"] = int(pts.size)
            res[f"{key}_bytes"] = int(ent.nbytes + pts.nbytes)
        res["blocks"] = int(kept["index_0"][1].size)
    for key, _ in variants:
        res[f"{key}_s"] = min(times[key])
        res[f"{key}_all_s"] = times[key]
    res["stream_bytes"] = len(stream)
    open(os.path.join(work, "stream.bz2"), "wb").write(stream)
    kept["index_256"][1].tofile(os.path.join(work, "entries.bin"))
    kept["index_256"][2].tofile(os.path.join(work, "points.bin"))
    return res


def step_oneshot(work):
    import numpy as np
    from banzai_amd import _native as nv
    data, _ = base.text()
    stream = open(os.path.join(work, "stream.bz2"), "rb").read()
    ent = np.fromfile(os.path.join(work, "entries.bin"), dtype=nv.INDEX_DTYPE)
    pts = np.fromfile(os.path.join(work, "points.bin"), dtype=nv.SYNC_DTYPE)

    def best(fn):
        ts = []
        for _ in range(REPS):
            t = time.perf_counter()
            r = fn()  # (host buffers in and out: the call has waited for the device when it returns)
            ts.append(time.perf_counter() - t)
        return min(ts), r

    with nv.Context(0, 9, 0) as ctx:
        ctx.encode_index(data, 256)  # warm-up
        t_enc, (s1, e1, p1) = best(lambda: ctx.encode_index(data, 256))
        assert s1 == stream and e1.tobytes() == ent.tobytes() and p1.tobytes() == pts.tobytes()
        ctx.decode_index_sync(stream, 256)  # warm-up
        t_dec, (e2, p2, _, used) = best(lambda: ctx.decode_index_sync(stream, 256))
    assert used == len(stream)
    assert e2.tobytes() == ent.tobytes() and p2.tobytes() == pts.tobytes(), "the streamed index differs from the decoder's"
    return {"encode_index_256_s": t_enc, "decode_index_sync_256_s": t_dec, "indexes_equal": True}


def table(res):
    s, o = res["stream"], res["oneshot"]
    ms = lambda v: f"{v * 1e3:.1f}"  # noqa: E731
    rows = [("`bzh_stream_begin`, 16 MiB feeds (the parent's path)", s["plain_s"], "-"),
            ("`bzh_stream_begin_index`, interval 256, a take after every feed", s["index_256_s"], f"{s['index_256_points']} points, {s['index_256_bytes']} bytes"),
            ("`bzh_stream_begin_index`, interval 0", s["index_0_s"], f"{s['blocks']} entries, {s['index_0_bytes']} bytes"),
            ("one-shot `bzh_encode_index`, interval 256 (whole input resident)", o["encode_index_256_s"], "the same arrays"),
            ("`bzh_decode_index_sync` of the stream, interval 256", o["decode_index_sync_256_s"], "the same arrays")]
    lines = ["| 100 MB text, level 9, host buffers | ms (best of 3) | index |", "|---|---|---|"]
    lines += [f"| {a} | {ms(b)} | {c} |" for a, b, c in rows]
    return "\n".join(lines)


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r19_gpu_stream_index.json")
    res = {}
    with tempfile.TemporaryDirectory() as work:
        for name, limit in STEPS:
            part = os.path.join(work, name + ".json")
            rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, work, part]).returncode
            if rc != 0:
                print(f"gpu_stream_index: step '{name}' ended with status {rc}; nothing further is started", flush=True)
                sys.exit(1)
            res[name] = json.load(open(part))
            os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
            with open(out, "w") as f:  # (after every step: a run that is cut short keeps what it measured)
                json.dump(res, f, indent=1)
            print(f"gpu_stream_index: step '{name}' done", flush=True)
    s, o = res["stream"], res["oneshot"]
    res["index_cost_s"] = s["index_256_s"] - s["plain_s"]
    res["alternative_s"] = s["plain_s"] + o["decode_index_sync_256_s"]
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(table(res))
    if not s["index_256_s"] < res["alternative_s"]:
        print("gpu_stream_index: the indexed stream is NOT cheaper than plain streaming plus the decode-side index build")
        sys.exit(1)


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "--step":
        json.dump({"stream": step_stream, "oneshot": step_oneshot}[sys.argv[2]](sys.argv[3]), open(sys.argv[4], "w"))
    else:
        main()
