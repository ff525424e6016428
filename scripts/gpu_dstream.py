"""The streaming decode on cuda:0, measured: python scripts/gpu_dstream.py [out.json]   (default profiles/r17_gpu_dstream.json)
Level 9, the 100 MB headline text of scripts/gpu_decode.py, host to host, best of 3 after a warm-up, on one context in one run:
  one shot : bzh_decode of the whole stream into a buffer of the decoded size;
  stream   : bzh_dstream_* at the default rooms, fed 8 MiB at a time, 16 MiB of room per call, with bzh_dstream_stats;
  small    : the same through a window of 4 MiB and a staging buffer of 16 MiB, to show what a pass costs.
Every step is a child process under a time limit of its own (the parent never opens the GPU); the first step that fails ends
the script.  Every decode is checked against the text."""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = (("encode", 300), ("decode", 400))  # (name, seconds)
REPS = 3
FEED, CAP = 8 << 20, 16 << 20


def text():
    from banzai_amd import corpus
    data, name = corpus.workload(100_000_000)
    return data.tobytes(), name


def step_encode(work):
    from banzai_amd import _native as nv
    data, name = text()
    with nv.Context(0, 9, 0) as ctx:
        stream = ctx.encode(data)
    open(os.path.join(work, "stream.bz2"), "wb").write(stream)
    return {"input": f"100 MB text ({name})", "level": 9, "stream_bytes": len(stream), "decoded_bytes": len(data)}


def best(fn):
    ts, r = [], None
    for _ in range(REPS):
        t = time.perf_counter()
        r = fn()
        ts.append(time.perf_counter() - t)
    return min(ts), r


def stream_decode(ctx, stream, out, buf, room):
    """the stream through bzh_dstream_* into `out` -> (bytes, stats)"""
    ctx.dstream_set_room(*room)
    ctx.dstream_begin()
    view, got, done = memoryview(stream), 0, False
    for at in range(0, len(stream), FEED):
        chunk, off, eof = view[at:at + FEED], 0, at + FEED >= len(stream)
        while not done:
            used, n, done = ctx.dstream_feed(chunk[off:], eof, buf)
            out[got:got + n] = buf[:n]
            got += n
            off += used
            if off == len(chunk) and n < buf.size and not eof:
                break
    assert done
    return got, ctx.dstream_stats()


def step_decode(work):
    import numpy as np
    from banzai_amd import _native as nv
    stream = open(os.path.join(work, "stream.bz2"), "rb").read()
    data, _ = text()
    truth = np.frombuffer(data, dtype=np.uint8)
    res = {"feed_bytes": FEED, "cap_bytes": CAP}
    with nv.Context(0, 9, 0) as ctx:
        st, out, need, used = ctx.decode_raw(stream, len(data))  # warm-up
        assert st == 0 and used == len(stream) and out == data
        t, _ = best(lambda: ctx.decode_raw(stream, len(data)))
        res["one_shot_s"] = t
        out = np.empty(len(data), dtype=np.uint8)
        buf = np.empty(CAP, dtype=np.uint8)
        for label, room in (("stream", (0, 0)), ("small", (4 << 20, 16 << 20))):
            got, _ = stream_decode(ctx, stream, out, buf, room)  # warm-up
            assert got == len(data) and np.array_equal(out, truth) and ctx.dstream_consumed() == len(stream)
            t, (got, stats) = best(lambda: stream_decode(ctx, stream, out, buf, room))
            assert got == len(data) and np.array_equal(out, truth)
            res[label] = {"window_target": room[0] or "default", "staging_target": room[1] or "default", "s": t,
                          "over_one_shot": t / res["one_shot_s"], "stats": stats}
        ctx.dstream_set_room(0, 0)
    return res


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r17_gpu_dstream.json")
    res = {"repeats": REPS}
    with tempfile.TemporaryDirectory() as work:
        for name, limit in STEPS:
            part = os.path.join(work, name + ".json")
            rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, work, part]).returncode
            if rc != 0:
                print(f"gpu_dstream: step '{name}' ended with status {rc}; nothing further is started", flush=True)
                sys.exit(1)
            res[name] = json.load(open(part))
            os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
            with open(out, "w") as f:  # (after every step: a run that is cut short keeps what it measured)
                json.dump(res, f, indent=1)
    d = res["decode"]
    print(f"one shot {d['one_shot_s'] * 1e3:.1f} ms")
    for label in ("stream", "small"):
        s = d[label]["stats"]
        print(f"{label}: {d[label]['s'] * 1e3:.1f} ms = {d[label]['over_one_shot']:.2f} x one shot; {s['passes']} passes, {s['blocks']} blocks, "
              f"{s['blocks_redone']} redone, window peak {s['window_peak']}, staging peak {s['staging_peak']}")


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "--step":
        result = {"encode": step_encode, "decode": step_decode}[sys.argv[2]](sys.argv[3])
        json.dump(result, open(sys.argv[4], "w"))
    else:
        main()
