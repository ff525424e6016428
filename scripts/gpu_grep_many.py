"""bzh_grep_many against the only way the library had before it, on cuda:0: python scripts/gpu_grep_many.py [out.json]
The workload: 4,096 x 4 KiB slices of the corpus text at level 9, encoded by bzh_encode_many_device, everything resident in HBM,
a rare word and a frequent one; after a warm-up five timed windows a step, each of 1 to 100 calls (INNER), so that a window
is far above the grain of the host clock; the least, the median and the greatest are written.
  (a) bzh_grep_many_device
  (b) a loop of bzh_grep_device, one call per input -- the parent commit's only way to the same answer
  (c) bzh_decode_many_device alone: what (a) pays before its segmented pass
  (r) bzh_grep_many_raw_device over the decoded bytes as 4,096 segments: the segmented pass alone
  (s) bzh_grep_raw_device over the same bytes as one text, on the same build: what the pass costs without walls
Every step is a child process under a time limit of its own; the first that fails ends the script.  Every step that greps per input
checks every input's count against Python's split-and-find of that slice.  Writes the JSON -- inputs/s of every step, (a)/(b),
(a) - (c), (r)/(s) and the share of tiles that several segments share -- and fails unless (a) is faster than (b)."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT, SIZE, LEVEL, REPS = 4096, 4096, 9, 5
INNER = {"a": 5, "b": 1, "c": 5, "r": 100, "s": 100}  # calls in one timed window
FREQUENT = b"the"


def child(step, which):
    import numpy as np  # noqa: F401
    import torch
    sys.path.insert(0, ROOT)
    from banzai_amd import _native as nv
    from banzai_amd import corpus

    text = corpus.workload(COUNT * SIZE)[0].tobytes()
    assert len(text) == COUNT * SIZE
    at = next(p for p in range(1_000_003, len(text)) if b"\n" not in text[p:p + 8])
    rare = text[at:at + 8]  # eight bytes of the text itself: they occur, and seldom
    word = rare if which == "rare" else FREQUENT
    assert b"\n" not in word
    slices = [text[k * SIZE:(k + 1) * SIZE] for k in range(COUNT)]
    want = [sum(word in ln for ln in s.split(b"\n")) for s in slices]  # (a line without its newline is a line)
    lens_in = [SIZE] * COUNT
    dev = torch.device("cuda", 0)

    inner = INNER[step]

    def timed(fn):
        """seconds a call: REPS timed windows of `inner` calls each (a window far above the clock's and a launch's grain) ->
        the least, the median and the greatest window, divided by the calls in it"""
        ts = []
        for _ in range(REPS):
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t) / inner)
        ts.sort()
        return ts[0], ts[len(ts) // 2], ts[-1]

    with nv.Context(0, LEVEL, 0) as ctx:
        d_text = torch.frombuffer(bytearray(text + b"\0" * 16), dtype=torch.uint8).to(dev)
        cap = nv.encode_many_bound(LEVEL, lens_in)
        d_comp = torch.zeros(cap + 16, dtype=torch.uint8, device=dev)
        offs, lens = ctx.encode_many_device(d_text.data_ptr(), lens_in, d_comp.data_ptr(), cap)
        n = offs[-1] + lens[-1]
        d_out = torch.zeros(len(text) + 64, dtype=torch.uint8, device=dev)
        row = {"step": step, "word": which, "pattern": word.decode("latin-1"), "inputs": COUNT, "stream_bytes": int(sum(lens)), "decoded_bytes": len(text),
               "selected_truth": int(sum(want))}
        seg_offs = [k * SIZE for k in range(COUNT)]
        if step == "a":
            st, nrecs, total, _, items = ctx.grep_many_device(d_comp.data_ptr(), n, offs, lens, word, 0, 0, 0)
            assert st == 0 and items["selected"].tolist() == want, "the counts of (a) differ from the split-and-find"

            def run():
                got = ctx.grep_many_device(d_comp.data_ptr(), n, offs, lens, word, d_out.data_ptr(), total, nrecs)
                assert got[:3] == (0, nrecs, total)
        elif step == "b":
            base_in, base_out, got_counts = d_comp.data_ptr(), d_out.data_ptr(), [0] * COUNT

            def run():
                for k in range(COUNT):
                    st, nr, _, _ = ctx.grep_device(base_in + offs[k], lens[k], word, base_out + k * SIZE, SIZE, 512)
                    assert st == 0
                    got_counts[k] = nr
        elif step == "c":
            def run():
                st, ooffs, olens, status, _ = ctx.decode_many_device(d_comp.data_ptr(), n, offs, lens, d_out.data_ptr(), len(text))
                assert st == 0 and not any(status) and olens == lens_in
        elif step == "r":
            st, nrecs, total, _, items = ctx.grep_many_raw_device(d_text.data_ptr(), len(text), seg_offs, lens_in, word, 0, 0, 0)
            assert st == 0 and items["selected"].tolist() == want, "the counts of (r) differ from the split-and-find"

            def run():
                got = ctx.grep_many_raw_device(d_text.data_ptr(), len(text), seg_offs, lens_in, word, d_out.data_ptr(), total, nrecs)
                assert got[:3] == (0, nrecs, total)
        else:  # s: one text, no walls (another answer: lines that cross a slice edge are whole)
            st, nrecs, total, _ = ctx.grep_raw_device(d_text.data_ptr(), len(text), word, 0, 0, 0)
            assert st == 0

            def run():
                got = ctx.grep_raw_device(d_text.data_ptr(), len(text), word, d_out.data_ptr(), total, nrecs)
                assert got[:3] == (0, nrecs, total)
        run()  # warm-up: code objects, the arena, the staging
        row["seconds"], row["seconds_median"], row["seconds_max"] = timed(run)
        row["calls_per_window"], row["windows"] = inner, REPS
        row["inputs_per_s"] = COUNT / row["seconds"]
        row["decoded_MB_per_s"] = len(text) / row["seconds"] / 1e6
        if step == "b":
            assert got_counts == want, "the counts of (b) differ from the split-and-find"
        if step in ("a", "r"):
            ms = ctx.grep_many_stats()
            row["many_stats"] = ms
            row["shared_tile_share"] = ms["shared_tiles"] / max(1, -(-len(text) // 4096))
            row["virtual_tiles_per_tile"] = ms["virtual_tiles"] / max(1, -(-len(text) // 4096))
    print("ROW " + json.dumps(row), flush=True)
    return 0


def step(name, which, limit=240):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, which], capture_output=True, text=True, timeout=limit)
    rows = [json.loads(line[4:]) for line in p.stdout.splitlines() if line.startswith("ROW ")]
    if p.returncode != 0 or not rows:
        print(f"step {name} ({which}) failed with exit status {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
        sys.exit(1)
    r = rows[0]
    print(f"({name}, {which}) {r['seconds'] * 1e3:.3f} ms (median {r['seconds_median'] * 1e3:.3f}, max {r['seconds_max'] * 1e3:.3f}; {r['windows']} windows of "
          f"{r['calls_per_window']} calls), {r['inputs_per_s']:.0f} inputs/s, {r['decoded_MB_per_s']:.0f} MB/s", flush=True)
    return r


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r33_gpu_grep_many.json")
    res = {"workload": f"{COUNT} x {SIZE} bytes of the corpus text, level {LEVEL}, device-resident, {REPS} windows of INNER calls after a warm-up: least, median, greatest"}
    res["c_decode_many_device"] = step("c", "rare")
    for which in ("rare", "frequent"):
        r = {"a_grep_many_device": step("a", which), "b_loop_of_grep_device": step("b", which, limit=420),
             "r_grep_many_raw_device": step("r", which), "s_grep_raw_device_one_text": step("s", which)}
        a, b, c = r["a_grep_many_device"]["seconds"], r["b_loop_of_grep_device"]["seconds"], res["c_decode_many_device"]["seconds"]
        r["a_over_b"] = b / a
        r["a_minus_c_ms"] = (a - c) * 1e3  # (least against least; the spread of both sides says how far to trust it)
        r["a_minus_c_ms_median"] = (r["a_grep_many_device"]["seconds_median"] - res["c_decode_many_device"]["seconds_median"]) * 1e3
        r["a_and_c_spread_ms"] = max(r["a_grep_many_device"]["seconds_max"] - a, res["c_decode_many_device"]["seconds_max"] - c) * 1e3
        r["r_over_s_median"] = r["r_grep_many_raw_device"]["seconds_median"] / r["s_grep_raw_device_one_text"]["seconds_median"]
        r["r_over_s"] = r["r_grep_many_raw_device"]["seconds"] / r["s_grep_raw_device_one_text"]["seconds"]
        r["shared_tile_share"] = r["r_grep_many_raw_device"]["shared_tile_share"]
        res[which] = r
        print(f"{which}: grep_many is {b / a:.1f}x the loop of grep_device; beside decode_many alone it costs {(a - c) * 1e3:.3f} ms; the segmented pass "
              f"is {r['r_over_s']:.2f}x the pass over one text, {r['shared_tile_share']:.2%} of the tiles are shared", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    if not all(res[w]["a_over_b"] > 1 for w in ("rare", "frequent")):
        sys.exit("bzh_grep_many_device is not faster than the loop of bzh_grep_device")


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--step":
        sys.exit(child(sys.argv[2], sys.argv[3]))
    main()
