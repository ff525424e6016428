"""The encoder's own index on cuda:0, measured: python scripts/gpu_encode_index.py [out.json]   (default profiles/r11_gpu_encode_index.json)
Level 9, the 100 MB headline text of scripts/gpu_index.py, everything resident in HBM, best of 3 after a warm-up:
  encode : (a) bzh_encode_device; (b) bzh_encode_index_device at intervals 0 and 256, same context, same buffers; the streams of
           all three are compared, the index is kept for the next step;
  decode : (c) bzh_decode_index_sync_device of that stream at interval 256 -- the existing way to the same index, the yardstick;
           its entries and points are compared with the encoder's, byte for byte.
The script fails unless (b at 256) - (a) is below (c).  Every step is a child process under a time limit of its own (the parent
never opens the GPU); the first step that fails ends the script."""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import gpu_index as base  # noqa: E402  (text, best)
import gpu_sync_index as sync  # noqa: E402  (index_sync_device)

STEPS = (("encode", 420), ("decode", 300))  # (name, seconds)


def step_encode(work):
    import torch
    from banzai_amd import _native as nv
    data, name = base.text()
    n = len(data)
    dev = torch.device("cuda", 0)
    d_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    cap = (n + n // 4 + (1 << 20)) & ~3
    d_out = torch.empty(cap, dtype=torch.uint8, device=dev)
    res = {"input": f"100 MB text ({name})", "level": 9, "repeats": base.REPS}
    with nv.Context(0, 9, 0) as ctx:
        ctx.encode_device(d_in.data_ptr(), n, d_out.data_ptr(), cap)  # warm-up
        t_enc, olen = base.best(lambda: ctx.encode_device(d_in.data_ptr(), n, d_out.data_ptr(), cap))
        stream = d_out[:olen].cpu().numpy().tobytes()
        res["encode_s"] = t_enc
        res["stream_bytes"] = olen
        for interval in (0, 256):
            max_e, max_p = nv.encode_index_bound(9, n, interval)
            call = lambda: ctx.encode_index_device(d_in.data_ptr(), n, d_out.data_ptr(), cap, interval, max_e, max_p)  # noqa: E731
            call()  # warm-up
            t, (olen2, ent, pts) = base.best(call)
            assert olen2 == olen and d_out[:olen].cpu().numpy().tobytes() == stream, interval
            res[f"encode_index_{interval}_s"] = t
            res[f"points_{interval}"] = int(pts.size)
            res[f"index_bytes_{interval}"] = int(ent.nbytes + pts.nbytes)
        res["blocks"] = int(ent.size)
        t_enc2, _ = base.best(lambda: ctx.encode_device(d_in.data_ptr(), n, d_out.data_ptr(), cap))  # (a) once more, behind (b)
        res["encode_again_s"] = t_enc2
    open(os.path.join(work, "stream.bz2"), "wb").write(stream)
    ent.copy().tofile(os.path.join(work, "entries.bin"))
    pts.copy().tofile(os.path.join(work, "points.bin"))
    return res


def step_decode(work):
    import numpy as np
    import torch
    from banzai_amd import _native as nv
    stream = open(os.path.join(work, "stream.bz2"), "rb").read()
    ent = np.fromfile(os.path.join(work, "entries.bin"), dtype=nv.INDEX_DTYPE)
    pts = np.fromfile(os.path.join(work, "points.bin"), dtype=nv.SYNC_DTYPE)
    d_in = torch.frombuffer(bytearray(stream), dtype=torch.uint8).to(torch.device("cuda", 0))
    with nv.Context(0, 9, 0) as ctx:
        sync.index_sync_device(ctx, d_in, len(stream), 256)  # warm-up; sizes the point array
        t, (ent2, pts2, total, used) = base.best(lambda: sync.index_sync_device(ctx, d_in, len(stream), 256))
    assert used == len(stream)
    assert ent2.tobytes() == ent.tobytes(), "the encoder's entries differ from the decoder's"
    assert pts2.tobytes() == pts.tobytes(), "the encoder's sync points differ from the decoder's"
    return {"decode_index_sync_s": t, "points": int(pts2.size), "index_bytes": int(ent2.nbytes + pts2.nbytes), "indexes_equal": True}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r11_gpu_encode_index.json")
    res = {}
    with tempfile.TemporaryDirectory() as work:
        for name, limit in STEPS:
            part = os.path.join(work, name + ".json")
            rc = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, work, part]).returncode
            if rc != 0:
                print(f"gpu_encode_index: step '{name}' ended with status {rc}; nothing further is started", flush=True)
                sys.exit(1)
            res[name] = json.load(open(part))
            os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
            with open(out, "w") as f:  # (after every step: a run that is cut short keeps what it measured)
                json.dump(res, f, indent=1)
            print(f"gpu_encode_index: step '{name}' done", flush=True)
    e, d = res["encode"], res["decode"]
    extra = e["encode_index_256_s"] - e["encode_s"]
    res["index_cost_s"] = extra
    res["decode_over_index_cost"] = d["decode_index_sync_s"] / extra if extra > 0 else None
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(f"encode {e['encode_s'] * 1e3:.3f} ms (again {e['encode_again_s'] * 1e3:.3f} ms), with entries {e['encode_index_0_s'] * 1e3:.3f} ms, "
          f"with {e['points_256']} points {e['encode_index_256_s'] * 1e3:.3f} ms ({e['index_bytes_256']} bytes); "
          f"the same index by decoding: {d['decode_index_sync_s'] * 1e3:.1f} ms")
    if not extra < d["decode_index_sync_s"]:
        print("gpu_encode_index: the index does NOT cost the encoder less than a decode pass")
        sys.exit(1)


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "--step":
        json.dump({"encode": step_encode, "decode": step_decode}[sys.argv[2]](sys.argv[3]), open(sys.argv[4], "w"))
    else:
        main()
