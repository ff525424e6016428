"""The encoder's launch sequence, for comparing two builds of the library kernel by kernel:
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/gpu_encode_launches.py run
      the branches of the encode driver once each on a 7-block level-1 input (the one of tests/test_gpu_encode_driver.py): one
      batch gated on the device, several batches on one lane, two lanes, a stream fed in pieces (passes of one batch and of
      several), two ranges and their assembly, the index hand-off of one batch and of several, many streams;
  python scripts/gpu_encode_launches.py list DIR > launches.txt
      the kernels of that trace in start order, one line each: name, grid, workgroup.
BZH_LIB names the library to load (default: the tree's)."""
import bz2
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run():
    import torch
    from banzai_amd import _native as nv
    from tests import cases
    big = cases.gen(360_000, "text", 31) + cases.gen(40_000, "longruns", 31) + cases.repeats(260_000, 31)
    two = big[:150_000]
    calls = 0

    def same(stream, data):
        nonlocal calls
        calls += 1
        assert bz2.decompress(stream) == data

    def fed(ctx, cuts):
        ctx.stream_begin(chunk_bytes=65536)
        out, pos = [], 0
        for c in cuts:
            out.append(ctx.stream_feed(big[pos:pos + c]))
            pos += c
        out.append(ctx.stream_feed(big[pos:], eof=True))
        return b"".join(out)

    with nv.Context(0, 1, 8) as c8, nv.Context(0, 1, 2) as c2, nv.Context(0, 1, 4) as c4:
        same(c8.encode(two), two)                                                     # a
        same(c8.encode(b"q"), b"q")
        same(c2.encode(big), big)                                                     # b
        c4.set_lanes(2)
        same(c4.encode(big), big)                                                     # c
        same(fed(c8, [100_001, 33_333, 170_000, 7, 120_000, 99_999]), big)            # d
        same(fed(c2, [400_000, 250_000]), big)
        cap = (len(big) + (1 << 16)) & ~3                                             # e
        d_in = torch.zeros(len(big) + 16, dtype=torch.uint8, device="cuda:0")
        d_in[:len(big)] = torch.frombuffer(bytearray(big), dtype=torch.uint8).to("cuda:0")
        bufs = [torch.zeros(cap, dtype=torch.uint8, device="cuda:0") for _ in range(3)]
        torch.cuda.synchronize()
        blocks = c2.plan_device(d_in.data_ptr(), len(big))
        segs = [(bufs[k].data_ptr(), c2.encode_range_device(b0, b1, bufs[k].data_ptr(), cap)) for k, (b0, b1) in enumerate(((0, 3), (3, len(blocks))))]
        ln = c2.assemble_device(segs, [b[3] for b in blocks], bufs[2].data_ptr(), cap)
        same(bufs[2][:ln].cpu().numpy().tobytes(), big)
        for ctx in (c8, c2):                                                          # f
            stream, ent, pts = ctx.encode_index(big, 16)
            same(stream, big)
        items = [b"", two[:40_000], big[:250_000], b"", two[:50_001], b"x" * 300, b""]  # g
        for got, item in zip(c2.encode_many(items), items):
            same(got, item)
        for got in c2.encode_many([b"", b""]):
            same(got, b"")
    print(f"gpu_encode_launches: {calls} streams over {len(blocks)} blocks, {len(ent)} entries, {len(pts)} sync points")


def listing(trace_dir):
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        rows += list(csv.DictReader(open(path)))
    # The encoder launches from several host threads (the lanes, a streaming pass) onto several streams (the suffix sort's side
    # streams), so start times interleave differently from run to run.  What a build decides is what each host thread
    # launches, in the order it does: one list per thread in dispatch order, the main thread's first, the others' by content.
    threads = {}
    for r in sorted(rows, key=lambda r: int(r["Dispatch_Id"])):
        threads.setdefault(r["Thread_Id"], []).append(
            f'{r["Kernel_Name"]} grid {r["Grid_Size_X"]}x{r["Grid_Size_Y"]}x{r["Grid_Size_Z"]} workgroup {r["Workgroup_Size_X"]}')
    lists = list(threads.values())
    for k, lines in enumerate(lists[:1] + sorted(lists[1:])):
        print(f"-- host thread {k}: {len(lines)} launches")
        print("\n".join(lines))


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) == 3 and sys.argv[1] == "list":
        listing(sys.argv[2])
    else:
        sys.exit(__doc__)
