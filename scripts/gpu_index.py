"""Random access on cuda:0, measured: python scripts/gpu_index.py [out.json]   (default profiles/r09_gpu_index.json)
Level 9, the 100 MB headline text of scripts/gpu_decode.py, everything resident in HBM, best of 3 after a warm-up:
  index : bzh_decode_index_device beside bzh_decode_device of the same stream on the same context in the same run, both with
          the stage times of bzh_decode_stats (one more run each with profiling on);
  range : bzh_decode_range_device of 4 KiB and of 1 MiB at 20 seeded offsets, median and worst, beside that same full decode.
Every step is a child process under a time limit of its own (the parent never opens the GPU); the first step that fails ends
the script.  The bytes of every range and the total of the index are checked against the text."""
import json
import os
import random
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = (("encode", 300), ("index", 300), ("range", 300))  # (name, seconds)
REPS = 3


def best(fn, reps=REPS):
    import torch
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return min(ts), r


def text():
    from banzai_amd import corpus
    data, name = corpus.workload(100_000_000)
    return data.tobytes(), name


def resident(stream, n_out):
    import torch
    dev = torch.device("cuda", 0)
    return torch.frombuffer(bytearray(stream), dtype=torch.uint8).to(dev), torch.empty(n_out + 64, dtype=torch.uint8, device=dev)


def full_decode(ctx, d_in, n_in, d_out):
    ctx.set_profiling(False)
    ctx.decode_device(d_in.data_ptr(), n_in, d_out.data_ptr(), d_out.numel())  # warm-up of this shape
    t, (got, used) = best(lambda: ctx.decode_device(d_in.data_ptr(), n_in, d_out.data_ptr(), d_out.numel()))
    ctx.set_profiling(True)
    ctx.decode_device(d_in.data_ptr(), n_in, d_out.data_ptr(), d_out.numel())
    st = ctx.decode_stats()
    ctx.set_profiling(False)
    return t, got, used, st


def step_encode(work):
    from banzai_amd import _native as nv
    data, name = text()
    with nv.Context(0, 9, 0) as ctx:
        stream = ctx.encode(data)
    open(os.path.join(work, "stream.bz2"), "wb").write(stream)
    return {"input": f"100 MB text ({name})", "level": 9, "stream_bytes": len(stream), "decoded_bytes": len(data)}


def index_device(ctx, d_in, n_in):
    import ctypes
    import numpy as np
    from banzai_amd import _native as nv
    ent = np.zeros(4096, dtype=nv.INDEX_DTYPE)
    cnt, used, total = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_uint64(0)
    ctx.check(nv.lib().bzh_decode_index_device(ctx.handle, ctypes.c_void_p(d_in.data_ptr()), n_in, ent.ctypes.data_as(nv.idxp), ent.size,
                                               ctypes.byref(cnt), ctypes.byref(total), ctypes.byref(used)))
    return ent[:cnt.value].copy(), int(total.value), int(used.value)


def step_index(work):
    from banzai_amd import _native as nv
    stream = open(os.path.join(work, "stream.bz2"), "rb").read()
    data, _ = text()
    d_in, d_out = resident(stream, len(data))
    with nv.Context(0, 9, 0) as ctx:
        t_full, got, used, st_full = full_decode(ctx, d_in, len(stream), d_out)
        assert got == len(data) and used == len(stream) and d_out[:got].cpu().numpy().tobytes() == data
        index_device(ctx, d_in, len(stream))  # warm-up
        t_idx, (ent, total, used) = best(lambda: index_device(ctx, d_in, len(stream)))
        assert total == len(data) and used == len(stream)
        ctx.set_profiling(True)
        index_device(ctx, d_in, len(stream))
        st_idx = ctx.decode_stats()
        ctx.set_profiling(False)
    ent.tofile(os.path.join(work, "index.bin"))
    return {"blocks": int(ent.size), "full_decode_s": t_full, "index_build_s": t_idx, "index_over_full": t_idx / t_full,
            "full_decode_stats": st_full, "index_build_stats": st_idx}


def step_range(work):
    import numpy as np
    from banzai_amd import _native as nv
    stream = open(os.path.join(work, "stream.bz2"), "rb").read()
    ent = np.fromfile(os.path.join(work, "index.bin"), dtype=nv.INDEX_DTYPE)
    data, _ = text()
    d_in, d_out = resident(stream, len(data))
    res = {}
    with nv.Context(0, 9, 0) as ctx:
        t_full, got, _, _ = full_decode(ctx, d_in, len(stream), d_out)
        assert got == len(data)
        res["full_decode_s"] = t_full
        rng = random.Random(9)
        for label, size in (("4KiB", 4096), ("1MiB", 1 << 20)):
            offs = [rng.randrange(len(data) - size) for _ in range(20)]
            ctx.decode_range_device(d_in.data_ptr(), len(stream), ent, offs[0], size, d_out.data_ptr(), size)  # warm-up
            times, blocks = [], []
            for off in offs:
                t, n = best(lambda: ctx.decode_range_device(d_in.data_ptr(), len(stream), ent, off, size, d_out.data_ptr(), size))
                assert n == size and d_out[:size].cpu().numpy().tobytes() == data[off:off + size], (label, off)
                times.append(t)
                blocks.append(ctx.decode_stats()["blocks"])
            ctx.set_profiling(True)
            ctx.decode_range_device(d_in.data_ptr(), len(stream), ent, offs[0], size, d_out.data_ptr(), size)
            st = ctx.decode_stats()
            ctx.set_profiling(False)
            res[label] = {"bytes": size, "offsets": offs, "blocks_touched": blocks, "median_s": statistics.median(times), "worst_s": max(times),
                          "full_over_median": t_full / statistics.median(times), "full_over_worst": t_full / max(times),
                          "stats_of_first_offset": st}
    return res


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r09_gpu_index.json")
    res = {"repeats": REPS}
    with tempfile.TemporaryDirectory() as work:
        for name, limit in STEPS:
            part = os.path.join(work, name + ".json")
            rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, work, part]).returncode
            if rc != 0:
                print(f"gpu_index: step '{name}' ended with status {rc}; nothing further is started", flush=True)
                sys.exit(1)
            res[name] = json.load(open(part))
            os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
            with open(out, "w") as f:  # (after every step: a run that is cut short keeps what it measured)
                json.dump(res, f, indent=1)
    i, r = res["index"], res["range"]
    print(f"index build {i['index_build_s'] * 1e3:.1f} ms, full decode {i['full_decode_s'] * 1e3:.1f} ms ({i['blocks']} blocks)")
    for label in ("4KiB", "1MiB"):
        print(f"{label} range: median {r[label]['median_s'] * 1e3:.2f} ms, worst {r[label]['worst_s'] * 1e3:.2f} ms; full decode "
              f"{r['full_decode_s'] * 1e3:.1f} ms = {r[label]['full_over_median']:.1f} x the median")


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "--step":
        result = {"encode": step_encode, "index": step_index, "range": step_range}[sys.argv[2]](sys.argv[3])
        json.dump(result, open(sys.argv[4], "w"))
    else:
        main()
