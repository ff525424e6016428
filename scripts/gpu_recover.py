"""bzh_recover* beside bzh_decode_device on cuda:0: python scripts/gpu_recover.py [out.json]
Everything resident in HBM, best of 3 after a warm-up, every step a child process under a time limit of its own; the first that
fails ends the script.  Every step compares what it wrote byte for byte.
  decode    bzh_decode_device of the 100 MB level-9 headline text's stream -- the yardstick: existing code
  recover   bzh_recover_device of the same undamaged stream
  damaged   bzh_recover_device with one payload bit flipped in each of 5 seeded blocks
  stream    bzh_recover_stream_device of the damaged stream's report, beside a device-to-device copy of as many bytes (its floor)
  many      4,096 x 4 KiB streams concatenated, through bzh_recover_device and bzh_recover_stream_device
Writes the JSON."""
import json
import os
import random
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, LEVEL, REPS = 100_000_000, 9, 3
COUNT, SIZE = 4096, 4096
STEPS = ("decode", "recover", "damaged", "stream", "many")


def child(step):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    from banzai_amd import _native as nv
    from banzai_amd import corpus

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

    def on_device(b):
        return torch.frombuffer(bytearray(bytes(b) + b"\0" * 16), dtype=torch.uint8).to(dev)

    row = {"step": step}
    with nv.Context(0, LEVEL, 0) as ctx:
        if step == "many":
            text = corpus.workload(COUNT * SIZE)[0].tobytes()
            lens_in = [SIZE] * COUNT
            d_text = on_device(text)
            cap = nv.encode_many_bound(LEVEL, lens_in)
            d_comp = torch.zeros(cap + 16, dtype=torch.uint8, device=dev)
            offs, lens = ctx.encode_many_device(d_text.data_ptr(), lens_in, d_comp.data_ptr(), cap)
            host = d_comp.cpu().numpy().tobytes()
            stream = b"".join(host[o:o + ln] for o, ln in zip(offs, lens))
        else:
            text = corpus.workload(N)[0].tobytes()
            d_text = on_device(text)
            cap = len(text) + len(text) // 4 + (1 << 20)
            d_comp = torch.zeros(cap, dtype=torch.uint8, device=dev)
            n = ctx.encode_device(d_text.data_ptr(), len(text), d_comp.data_ptr(), cap)
            stream = d_comp[:n].cpu().numpy().tobytes()
        del d_text
        row.update(stream_bytes=len(stream), decoded_bytes=len(text))
        want = text
        if step in ("damaged", "stream"):  # one bit in the last fifth of each of 5 seeded blocks
            idx, _, _ = ctx.decode_index(stream)
            rng = random.Random(20261019)
            hit = sorted(rng.sample(range(len(idx)), 5))
            b = bytearray(stream)
            for k in hit:
                at = int(idx["bit_pos"][k]) + int((int(idx["end_bit"][k]) - int(idx["bit_pos"][k])) * 0.8) + rng.randrange(64)
                b[at // 8] ^= 0x80 >> (at % 8)
            stream = bytes(b)
            want = b"".join(text[int(e["out_off"]):int(e["out_off"]) + int(e["out_len"])] for k, e in enumerate(idx) if k not in hit)
            row.update(blocks=len(idx), blocks_hit=hit)
        d_in = on_device(stream)
        d_out = torch.zeros(len(text) + 64, dtype=torch.uint8, device=dev)
        max_ent = len(stream) // 1000 + 8192  # (room for every block of either workload: a 4 KiB stream is some 1,600 bytes)
        if step == "decode":
            def run():
                got, used = ctx.decode_device(d_in.data_ptr(), len(stream), d_out.data_ptr(), len(text))
                assert got == len(text) and used == len(stream)
        else:
            def run():
                st, need, ent, cnt = ctx.recover_device(d_in.data_ptr(), len(stream), d_out.data_ptr(), len(text), max_ent)
                assert st == 0 and need == len(want), (st, need, len(want))
                run.ent = ent
        run()  # warm-up: code objects, the arena
        d_out.zero_()
        row["seconds"] = timed(run)
        row["identical"] = d_out[:len(want)].cpu().numpy().tobytes() == want
        row["decoded_MB_per_s"] = len(want) / row["seconds"] / 1e6
        if step != "decode":
            row["recover_stats"] = ctx.recover_stats()
            row["lost"] = int((run.ent["kind"] != 0).sum())
        ctx.set_profiling(True)
        run()
        row["stages_ms"] = {k: v for k, v in ctx.decode_stats().items() if k.startswith("ms_")}
        ctx.set_profiling(False)
        if step in ("stream", "many"):
            ent = run.ent
            kept = ent[ent["kind"] == 0]
            bits = int((kept["end_bit"].astype(object) - kept["bit_pos"].astype(object)).sum())
            size = 4 + (bits + 80 + 7) // 8
            room = (size + 3) // 4 * 4
            d_rep = torch.zeros(room + 16, dtype=torch.uint8, device=dev)
            d_src = torch.zeros(room, dtype=torch.uint8, device=dev)

            def gather():
                st, need = ctx.recover_stream_device(d_in.data_ptr(), len(stream), ent, d_rep.data_ptr(), room)
                assert (st, need) == (0, size), (st, need, size)

            def copy():
                d_rep[:room].copy_(d_src)
            copy()
            row["copy_seconds"] = timed(copy)
            gather()
            row["stream_seconds"] = timed(gather)
            row["repaired_bytes"] = size
            row["kept_blocks"] = int(kept.size)
            row["stream_GB_per_s"] = size / row["stream_seconds"] / 1e9
            row["copy_GB_per_s"] = room / row["copy_seconds"] / 1e9
            # the repaired stream decodes, on the GPU, to the salvage
            d_out.zero_()
            got, used = ctx.decode_device(d_rep.data_ptr(), size, d_out.data_ptr(), len(text))
            row["repaired_identical"] = got == len(want) and used == size and d_out[:len(want)].cpu().numpy().tobytes() == want
    print("ROW " + json.dumps(row), flush=True)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    rows = []
    for step in STEPS:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", step], capture_output=True, text=True, timeout=420)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("ROW ")]
        if p.returncode != 0 or not line:
            print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
            sys.exit(f"step {step}: exit status {p.returncode}")
        rows.append(json.loads(line[0][4:]))
        print(json.dumps(rows[-1]), flush=True)
        if not rows[-1]["identical"] or rows[-1].get("repaired_identical") is False:
            sys.exit(f"step {step}: the output differs")
    result = {"workload": f"{N} bytes of the headline text at level {LEVEL}; {COUNT} x {SIZE}-byte streams", "best_of": REPS, "rows": rows}
    if out_path:
        with open(out_path, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        main()
