"""Sync points on cuda:0, measured: python scripts/gpu_sync_index.py [out.json]   (default profiles/r10_gpu_sync.json)
Level 9, the 100 MB headline text of scripts/gpu_index.py, everything resident in HBM, best of 3 after a warm-up:
  index : bzh_decode_index_sync_device at interval 256 beside bzh_decode_index_device, same stream, same context, with the
          stage times of bzh_decode_stats (one more run each with profiling on) and the size of the index in bytes;
  range : bzh_decode_range_sync_device of 4 KiB and of 1 MiB at 20 seeded offsets, median and worst, beside
          bzh_decode_range_device at the same offsets on the same context (the yardstick: the un-synced path of the same
          build); the whole range [0, total) both ways beside bzh_decode_device; ms_entropy of each;
  range64 / range1024 : the same reads with the points of intervals 64 and 1024.
Every step is a child process under a time limit of its own (the parent never opens the GPU); the first step that fails ends
the script.  The bytes of every range are checked against the text."""
import ctypes
import json
import os
import random
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import gpu_index as base  # noqa: E402  (text, resident, best, full_decode, index_device, step_encode)

STEPS = (("encode", 300), ("index", 300), ("range", 420), ("range64", 300), ("range1024", 300))  # (name, seconds)
REPS = base.REPS


def index_sync_device(ctx, d_in, n_in, interval):
    """bzh_decode_index_sync_device: one call sizes, one fills (the timed unit is the pair's second call: see step_index)"""
    import numpy as np
    from banzai_amd import _native as nv
    ent = np.zeros(4096, dtype=nv.INDEX_DTYPE)
    pts = np.zeros(index_sync_device.room, dtype=nv.SYNC_DTYPE)
    cnt, npts, used, total = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_uint64(0)
    st = nv.lib().bzh_decode_index_sync_device(ctx.handle, ctypes.c_void_p(d_in.data_ptr()), n_in, interval, ent.ctypes.data_as(nv.idxp),
                                               ent.size, ctypes.byref(cnt), pts.ctypes.data_as(nv.syncp) if pts.size else None, pts.size,
                                               ctypes.byref(npts), ctypes.byref(total), ctypes.byref(used))
    if st == -4 and npts.value > pts.size:  # (the first call of a run: room for the points from now on)
        index_sync_device.room = npts.value
        return index_sync_device(ctx, d_in, n_in, interval)
    ctx.check(st)
    return ent[:cnt.value].copy(), pts[:npts.value].copy(), int(total.value), int(used.value)


index_sync_device.room = 0


def profiled(ctx, fn):
    ctx.set_profiling(True)
    fn()
    st = ctx.decode_stats()
    ctx.set_profiling(False)
    return st


def step_index(work):
    from banzai_amd import _native as nv
    stream = open(os.path.join(work, "stream.bz2"), "rb").read()
    data, _ = base.text()
    d_in, d_out = base.resident(stream, len(data))
    with nv.Context(0, 9, 0) as ctx:
        base.index_device(ctx, d_in, len(stream))  # warm-up
        t_idx, (ent, total, used) = base.best(lambda: base.index_device(ctx, d_in, len(stream)))
        assert total == len(data) and used == len(stream)
        st_idx = profiled(ctx, lambda: base.index_device(ctx, d_in, len(stream)))
        index_sync_device(ctx, d_in, len(stream), 256)  # warm-up; sizes the point array, so that a timed call is one build
        t_sync, (ent2, pts, total2, _) = base.best(lambda: index_sync_device(ctx, d_in, len(stream), 256))
        assert ent2.tobytes() == ent.tobytes() and total2 == total
        st_sync = profiled(ctx, lambda: index_sync_device(ctx, d_in, len(stream), 256))
    ent.tofile(os.path.join(work, "index.bin"))
    return {"blocks": int(ent.size), "interval": 256, "points": int(pts.size), "index_build_s": t_idx, "index_sync_build_s": t_sync,
            "sync_over_plain": t_sync / t_idx, "index_bytes": int(ent.nbytes), "sync_index_bytes": int(ent.nbytes + pts.nbytes),
            "index_build_stats": st_idx, "index_sync_build_stats": st_sync}


def reads(ctx, call, data, d_out, plan):
    """plan: [(label, size, offsets)] -> {label: median / worst / ms_entropy of the first offset}"""
    res = {}
    for label, size, offs in plan:
        call(offs[0], size)  # warm-up
        times = []
        for off in offs:
            t, n = base.best(lambda: call(off, size))
            want = data[off:off + size]
            assert n == len(want) and d_out[:n].cpu().numpy().tobytes() == want, (label, off)
            times.append(t)
        st = profiled(ctx, lambda: call(offs[0], size))
        res[label] = {"bytes": size, "median_s": statistics.median(times), "worst_s": max(times), "ms_entropy": st["ms_entropy"],
                      "blocks_of_first_offset": st["blocks"], "stats_of_first_offset": st}
    return res


def read_plan(data):
    rng = random.Random(9)
    plan = []
    for label, size in (("4KiB", 4096), ("1MiB", 1 << 20)):
        plan.append((label, size, [rng.randrange(len(data) - size) for _ in range(20)]))
    plan.append(("whole", len(data), [0]))
    return plan


def step_range(work, interval=256, yardstick=True):
    import numpy as np
    from banzai_amd import _native as nv
    stream = open(os.path.join(work, "stream.bz2"), "rb").read()
    ent = np.fromfile(os.path.join(work, "index.bin"), dtype=nv.INDEX_DTYPE)
    data, _ = base.text()
    d_in, d_out = base.resident(stream, len(data))
    res = {"interval": interval}
    with nv.Context(0, 9, 0) as ctx:
        ent2, pts, _, _ = index_sync_device(ctx, d_in, len(stream), interval)
        assert ent2.tobytes() == ent.tobytes()
        res["points"] = int(pts.size)
        res["sync_index_bytes"] = int(ent.nbytes + pts.nbytes)
        plan = read_plan(data)
        res["offsets"] = {label: offs for label, _, offs in plan}
        res["sync"] = reads(ctx, lambda off, size: ctx.decode_range_sync_device(d_in.data_ptr(), len(stream), ent, pts, off, size,
                                                                                d_out.data_ptr(), size), data, d_out, plan)
        if yardstick:
            res["plain"] = reads(ctx, lambda off, size: ctx.decode_range_device(d_in.data_ptr(), len(stream), ent, off, size, d_out.data_ptr(),
                                                                                size), data, d_out, plan)
            t_full, got, _, st_full = base.full_decode(ctx, d_in, len(stream), d_out)
            assert got == len(data)
            res["full_decode_s"] = t_full
            res["full_decode_ms_entropy"] = st_full["ms_entropy"]
            for label in ("4KiB", "1MiB", "whole"):
                res["sync"][label]["plain_over_sync_median"] = res["plain"][label]["median_s"] / res["sync"][label]["median_s"]
    return res


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r10_gpu_sync.json")
    res = {"repeats": REPS}
    with tempfile.TemporaryDirectory() as work:
        for name, limit in STEPS:
            part = os.path.join(work, name + ".json")
            rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, work, part]).returncode
            if rc != 0:
                print(f"gpu_sync_index: step '{name}' ended with status {rc}; nothing further is started", flush=True)
                sys.exit(1)
            res[name] = json.load(open(part))
            os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
            with open(out, "w") as f:  # (after every step: a run that is cut short keeps what it measured)
                json.dump(res, f, indent=1)
            print(f"gpu_sync_index: step '{name}' done", flush=True)
    i, r = res["index"], res["range"]
    print(f"index build {i['index_build_s'] * 1e3:.1f} ms, with sync points {i['index_sync_build_s'] * 1e3:.1f} ms "
          f"({i['blocks']} blocks, {i['points']} points, {i['sync_index_bytes']} bytes)")
    for key in ("range", "range64", "range1024"):
        for label in ("4KiB", "1MiB", "whole"):
            s = res[key]["sync"][label]
            line = f"interval {res[key]['interval']:4d} {label:5s}: median {s['median_s'] * 1e3:8.2f} ms, worst {s['worst_s'] * 1e3:8.2f} ms, entropy {s['ms_entropy']:.2f} ms"
            if "plain" in res[key]:
                p = res[key]["plain"][label]
                line += f"; un-synced median {p['median_s'] * 1e3:8.2f} ms, worst {p['worst_s'] * 1e3:8.2f} ms, entropy {p['ms_entropy']:.2f} ms"
            print(line)
    print(f"full decode {r['full_decode_s'] * 1e3:.1f} ms (entropy {r['full_decode_ms_entropy']:.1f} ms)")
    if not r["sync"]["4KiB"]["median_s"] < r["plain"]["4KiB"]["median_s"]:
        print("gpu_sync_index: the 4 KiB median with sync points is NOT below the one without")
        sys.exit(1)


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "--step":
        steps = {"encode": base.step_encode, "index": step_index, "range": step_range,
                 "range64": lambda w: step_range(w, 64, False), "range1024": lambda w: step_range(w, 1024, False)}
        json.dump(steps[sys.argv[2]](sys.argv[3]), open(sys.argv[4], "w"))
    else:
        main()
