"""bzh_decode_many against the ways the library had before it, on cuda:0: python scripts/gpu_decode_many.py [out.json]
The workload: 4,096 x 4 KiB slices of the corpus text at level 9, encoded by bzh_encode_many_device, everything resident in HBM,
best of 3 after a warm-up.
  (a) a loop of bzh_decode_device, one call per stream -- the only way to per-input results before bzh_decode_many
  (b) one bzh_decode_device over the streams concatenated without padding -- the best case before it, with no isolation
  (c) bzh_decode_many_device
  (d) (c) with the LDS inverse BWT switched off (BZH_UNBWT_SMALL=0)
then (c) and (d) in five alternating runs each for the kernel's place, judged on ms_unbwt by the yardstick of
profiles/r08_mtf_emit_ab.txt: every run of one side faster than every run of the other.  Every step is a child process under a
time limit of its own; the first that fails ends the script.  Every step compares its output with the input byte for byte.
Writes the JSON, and fails unless (c) is faster than (a)."""
import json
import math
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT, SIZE, LEVEL, REPS = 4096, 4096, 9, 3


def child(step):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from banzai_amd import _native as nv
    from banzai_amd import corpus

    text = corpus.workload(COUNT * SIZE)[0].tobytes()
    assert len(text) == COUNT * SIZE
    lens_in = [SIZE] * COUNT
    dev = torch.device("cuda", 0)

    def timed(fn):
        ts = []
        for _ in range(REPS):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t)
        return min(ts)

    with nv.Context(0, LEVEL, 0) as ctx:
        d_text = torch.frombuffer(bytearray(text + b"\0" * 16), dtype=torch.uint8).to(dev)
        cap = nv.encode_many_bound(LEVEL, lens_in)
        d_comp = torch.zeros(cap + 16, dtype=torch.uint8, device=dev)
        offs, lens = ctx.encode_many_device(d_text.data_ptr(), lens_in, d_comp.data_ptr(), cap)
        n = offs[-1] + lens[-1]
        d_out = torch.zeros(len(text) + 64, dtype=torch.uint8, device=dev)
        row = {"step": step, "streams": COUNT, "stream_bytes": int(sum(lens)), "decoded_bytes": len(text)}
        if step == "a":
            base_in, base_out = d_comp.data_ptr(), d_out.data_ptr()

            def run():
                for k in range(COUNT):
                    got, _ = ctx.decode_device(base_in + offs[k], lens[k], base_out + k * SIZE, SIZE)
                    assert got == SIZE
        elif step == "b":
            host = d_comp.cpu().numpy().tobytes()
            cat = b"".join(host[o:o + ln] for o, ln in zip(offs, lens))
            d_cat = torch.frombuffer(bytearray(cat + b"\0" * 16), dtype=torch.uint8).to(dev)

            def run():
                got, used = ctx.decode_device(d_cat.data_ptr(), len(cat), d_out.data_ptr(), len(text))
                assert got == len(text) and used == len(cat)
        else:  # c, d (the parent sets the switch in the environment)
            def run():
                st, ooffs, olens, status, _ = ctx.decode_many_device(d_comp.data_ptr(), n, offs, lens, d_out.data_ptr(), len(text))
                assert st == 0 and not any(status) and olens == lens_in and ooffs[-1] == len(text) - SIZE
        run()  # warm-up: code objects, the arena
        d_out.zero_()
        row["seconds"] = timed(run)
        row["identical"] = d_out[:len(text)].cpu().numpy().tobytes() == text
        row["streams_per_s"] = COUNT / row["seconds"]
        row["decoded_MB_per_s"] = len(text) / row["seconds"] / 1e6
        if step in ("b", "c", "d"):
            ctx.set_profiling(True)
            prof = []
            for _ in range(REPS):
                run()
                prof.append((ctx.decode_stats(), ctx.decode_many_stats()))
            ctx.set_profiling(False)
            ds, ms = min(prof, key=lambda p: p[0]["ms_unbwt"])
            row["stats"] = ds
            row["ms_unbwt"] = ds["ms_unbwt"]
            if step != "b":
                row["many_stats"] = ms
                row["ms_unbwt_small"] = ms["ms_unbwt_small"]
                row["batches"] = ms["batches"]
                # launches of the inverse BWT a batch: the LDS path is one; unbwt_run is byte_count, active_bases, one radix
                # pass, unbwt_init, a round per doubling of the longest block (4 KiB of text stays 4 KiB behind RLE1) and unbwt_emit
                row["unbwt_launches_per_batch"] = 1 if ms["blocks_small"] else 5 + int(math.log2(SIZE)) + 1
    print("ROW " + json.dumps(row), flush=True)
    return 0 if row["identical"] else 1


def step(name, lds_off=False, limit=240):
    env = dict(os.environ)
    env.pop("BZH_UNBWT_SMALL", None)
    if lds_off:
        env["BZH_UNBWT_SMALL"] = "0"
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name], env=env, capture_output=True, text=True, timeout=limit)
    rows = [json.loads(line[4:]) for line in p.stdout.splitlines() if line.startswith("ROW ")]
    if p.returncode != 0 or not rows:
        print(f"step {name} failed with exit status {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
        sys.exit(1)
    r = rows[0]
    print(f"({name}{' LDS off' if lds_off else ''}) {r['seconds'] * 1e3:.2f} ms, {r['streams_per_s']:.0f} streams/s, {r['decoded_MB_per_s']:.0f} MB/s"
          + (f", ms_unbwt {r['ms_unbwt']:.3f}" if "ms_unbwt" in r else "") + (f", ms_unbwt_small {r['ms_unbwt_small']:.3f}, batches {r['batches']}"
                                                                             if "batches" in r else ""), flush=True)
    return r


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r13_gpu_decode_many.json")
    res = {"workload": f"{COUNT} x {SIZE} bytes of the corpus text, level {LEVEL}, device-resident, best of {REPS} after a warm-up",
           "a_loop_of_decode_device": step("a", limit=420), "b_one_decode_of_the_concatenation": step("b"),
           "c_decode_many_device": step("c"), "d_decode_many_device_lds_off": step("d", lds_off=True), "ab": []}
    for k in range(5):  # (c) and (d) alternating: the kernel's place
        res["ab"].append({"lds": "on", **{f: v for f, v in step("c").items() if f in ("seconds", "ms_unbwt", "ms_unbwt_small")}})
        res["ab"].append({"lds": "off", **{f: v for f, v in step("d", lds_off=True).items() if f in ("seconds", "ms_unbwt", "ms_unbwt_small")}})
    on = [r["ms_unbwt"] for r in res["ab"] if r["lds"] == "on"]
    off = [r["ms_unbwt"] for r in res["ab"] if r["lds"] == "off"]
    res["lds_wins_every_run_on_ms_unbwt"] = max(on) < min(off)
    res["lds_loses_every_run_on_ms_unbwt"] = min(on) > max(off)
    a, b, c = (res[k]["seconds"] for k in ("a_loop_of_decode_device", "b_one_decode_of_the_concatenation", "c_decode_many_device"))
    res["c_over_a"] = a / c
    res["c_over_b"] = b / c  # recorded; it decides nothing
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"decode_many is {a / c:.1f}x the loop of decode_device and {b / c:.2f}x the one decode of the concatenation; ms_unbwt LDS on "
          f"{min(on):.3f}..{max(on):.3f}, off {min(off):.3f}..{max(off):.3f}")
    if not all(res[k]["identical"] for k in res if isinstance(res[k], dict) and "identical" in res[k]):
        sys.exit("an output differs from the input")
    if not c < a:
        sys.exit("bzh_decode_many_device is not faster than the loop of bzh_decode_device")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--step":
        sys.exit(child(sys.argv[2]))
    main()
