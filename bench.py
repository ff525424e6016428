#!/usr/bin/env python3
"""bench.py -- encode MB/s (input) at level 9 on enwik8(-synthetic), 1/2/4/8 MI355X.

A "step" = one pass of the whole hot path (RLE1 split -> BWT -> MTF/RLE2 -> Huffman -> bit pack ->
stream assembly) over the workload, inputs resident in HBM when the timed region starts, the
finished .bz2 stream resident in HBM on rank 0 when it ends.

N = 1: 100,000,000 bytes (BASELINE.json configs[2]) through bzh_encode_device.
N > 1: weak scaling, N x 100,000,000 bytes as ONE stream (`--total-bytes 1000000000` instead runs BASELINE.json's
config 4, one 1 GB stream over the N ranks).  `python bench.py --gpus N` without a launcher starts its own ranks
(a fresh `python -m torch.distributed.run` child, before this process touches the GPU); under a launcher
(WORLD_SIZE set) it is one rank.  Rank r holds its own byte range plus a look-ahead (sharded.resident_range),
builds the split's tables over it, receives the start of its first block from rank r-1 (8 bytes), cuts and
encodes the blocks that start in its range; the encoded bit strings are gathered to rank 0 over RCCL
(torch.distributed backend "nccl") and funnel-shifted into the stream there.

Timed region: K steps with profiling OFF (the product's default path).

A plain run does only what the headline needs: it sets up, takes one first-touch step (the library sizes its arena) and
the W warm-up steps, times the K steps and prints ONE JSON line on rank 0 (`metric`, `value`, `unit`, `ms_per_step`,
`higher_is_better`, `dtype`, the configuration and `compressed_bytes`).  `--dump-outputs DIR` writes the stream of the
last timed step beside it (dump_outputs).  Everything else is measured and checked with `--full` only, as follows.

Stage timings, the radix-pass roofline (HIP events on the context's stream) and the counters of `roofline.path_frac`
come from a second, untimed pass of the same K steps with profiling on.

Output with --full: ONE JSON line on rank 0 (see the driver contract) with `roofline` (the kernel class that took the most time
in the profiled pass -- chunk_finish since the bucket-first initial sort -- its launches timed by HIP events on the
stream it runs on, the ten most expensive classes beside it, and the whole path by SURVEY 8(d)'s fixed accounting),
`cpu_baseline` (the oracle =
single-thread C restatement of banzai's path, timed on the same workload; also the bit-exactness
check), `value_host_inclusive` (pinned host buffers through bzh_encode, PCIe inside the clock), `value_stream_api` (the
reference's API surface: the streaming entry points fed from pageable memory, C ABI and banzai_amd.encode),
`value_real_text` and `extra_workloads` (round 1-3's generator, real files of the image with their SHA-256 + the four
C5 parts, each bit-exact vs the oracle; the oracle legs run on a thread pool).
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

SEGMENT = 100_000_000          # bytes per GPU (enwik8 size)
LEVEL = 9
HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
SORT_BYTES_PER_ELEM = 16.0     # one radix pass moves an 8-byte (key, suffix) pair: read 8 + write 8
METRIC = "encode MB/s (input) at level 9, enwik8, 1/2/4/8 MI355X; bit-exact vs CPU"
DUMP_BYTES = 8_000_000         # stream bytes --dump-outputs writes at most (as float32: 32 MB of the 64 MB allowed)
DUMP_PIECE = 1 << 20           # --dump-outputs sums the stream per piece of this many bytes
DUMP_SEED = 20061


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bytes", type=int, default=SEGMENT, help="bytes per GPU")
    ap.add_argument("--total-bytes", type=int, default=0,
                    help="size of the ONE stream all ranks share (overrides --bytes; 1000000000 = BASELINE config 4)")
    ap.add_argument("--full", action="store_true",
                    help="beside the headline: the profiled pass (stage times, roofline), the checks, the oracle "
                         "(cpu_baseline) and the other workloads and entry points")
    ap.add_argument("--dump-outputs", metavar="DIR", default="",
                    help="after the timed steps, write the stream of the last one to DIR/*.npy (see dump_outputs)")
    ap.add_argument("--cpu-sample", type=int, default=100_000_000, help="--full: bytes of the workload timed on the CPU oracle")
    ap.add_argument("--no-cpu", action="store_true", help="--full: skip the oracle (no cpu_baseline, no bit-exactness checks)")
    ap.add_argument("--no-extra", action="store_true", help="--full: skip extra_workloads and value_host_inclusive")
    ap.add_argument("--single-process", action="store_true",
                    help="--gpus N inside ONE process: bzh_create_multi (one host thread and context per device inside the "
                         "library) instead of one rank per GPU over torch.distributed")
    ap.add_argument("--devices", default="", help="--single-process: the device list, e.g. 0,0,0 (default 0..N-1)")
    return ap.parse_args()


def self_launch(args):
    """--gpus N without a launcher: start N fresh ranks.  Nothing in this process has touched the GPU yet
    (no torch.cuda / HIP call), and it never does: it only waits for the child and passes its exit code on."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    # HSA_ENABLE_IPC_MODE_LEGACY=0: the host driver of this pool only supports dmabuf IPC; with the legacy mode RCCL's
    # cross-process buffer registration fails with "hipIpcGetMemHandle: invalid argument" (the image exports the variable
    # already; a launch from a stripped environment must not lose it)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return subprocess.call(cmd, env=env)


def path_alg_bytes(st):
    """B_alg = N_in + 97 n + 96 A + 6 m + 3 o (bytes), from the counters of one step."""
    return (st["raw_bytes"] + 97 * st["rle_bytes"] + 96 * st["bwt_active_sum"] + 6 * st["mtf_syms"]
            + 3 * ((st["out_bits"] + 7) // 8))


def dump_outputs(out_dir, stream):
    """--dump-outputs: what a caller of the timed path receives, the .bz2 stream (uint8), as float arrays that two builds
    can be compared by, file for file:
      stream_length.npy       float64 [1]: its length in bytes
      stream_bytes.npy        float32: every byte if there are at most DUMP_BYTES, else the bytes at DUMP_BYTES positions
                              drawn with DUMP_SEED (sorted, the same positions for the same length)
      stream_piece_sums.npy   float64 [pieces, 2]: the sum and the position-weighted sum (weights 1, 2, ...) of the bytes of
                              every DUMP_PIECE-byte piece, which every byte enters (integers below 2^53: exact)"""
    import numpy as np
    s = np.asarray(stream, dtype=np.uint8).reshape(-1)
    n = int(s.size)
    if n > DUMP_BYTES:
        s_out = s[np.sort(np.random.default_rng(DUMP_SEED).integers(0, n, DUMP_BYTES))]
    else:
        s_out = s
    w = np.arange(1, DUMP_PIECE + 1, dtype=np.float64)
    sums = np.zeros((-(-n // DUMP_PIECE), 2), dtype=np.float64)
    for k in range(sums.shape[0]):
        p = s[k * DUMP_PIECE:(k + 1) * DUMP_PIECE].astype(np.float64)
        sums[k] = (p.sum(), p @ w[:p.size])
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "stream_length.npy"), np.array([n], dtype=np.float64))
    np.save(os.path.join(out_dir, "stream_bytes.npy"), s_out.astype(np.float32))
    np.save(os.path.join(out_dir, "stream_piece_sums.npy"), sums)


def single_process(args):
    """--gpus N --single-process: the N devices behind ONE handle (bzh_create_multi, include/bzhip.h) -- what a caller of
    banzai_amd.encode(..., devices=[...]) / bnzhip with $BZHIP_DEVICES runs.  Same line shape as the launcher flow; a step
    is bzh_multi_run: every worker's byte range resident on its device when it starts, the stream resident on the first
    device when it ends."""
    import bz2
    import numpy as np
    import torch
    from banzai_amd import _native as nv
    from banzai_amd import corpus
    world = args.gpus
    devices = [int(x) for x in args.devices.split(",")] if args.devices else list(range(world))
    if len(devices) != world:
        raise SystemExit(f"--devices lists {len(devices)} devices, --gpus says {world}")
    total = args.total_bytes or args.bytes * world
    seg_bytes = -(-total // world)
    segs, wname = [], None
    for k in range(world):
        sl = max(0, min(seg_bytes, total - k * seg_bytes))
        sk, wname = corpus.workload(max(1, sl), segment=k)
        segs.append(sk[:sl])
    data = np.concatenate(segs)
    with nv.MultiContext(devices, LEVEL) as m:
        m.load(data)
        out_len = m.run()
        for _ in range(args.warmup):
            out_len = m.run()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out_len = m.run()
        dt = time.perf_counter() - t0
        per_worker = m.times()
        stream = m.fetch(out_len)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, np.frombuffer(stream, dtype=np.uint8))
    checks = {}
    if args.full:
        if total <= 200_000_000:
            checks["libbz2_roundtrip"] = bool(bz2.decompress(stream) == data.tobytes())
        dev = torch.device("cuda", devices[0])
        with nv.Context(devices[0], LEVEL) as ctx:
            d_in = torch.zeros(total + 16, dtype=torch.uint8, device=dev)
            d_in[:total] = torch.from_numpy(data).to(dev)
            cap = (total // 3 + total // 8 + (1 << 20)) & ~3
            d_out = torch.zeros(cap, dtype=torch.uint8, device=dev)
            ln = ctx.encode_device(d_in.data_ptr(), total, d_out.data_ptr(), cap)
            checks["sharded_equals_single_gpu"] = bool(d_out[:ln].cpu().numpy().tobytes() == stream)
    ms = dt * 1e3 / args.steps
    result = {"metric": METRIC, "value": round(total * args.steps / dt / 1e6, 2), "unit": "MB/s", "n_gpus": world, "steps": args.steps,
              "warmup": args.warmup, "ms_per_step": round(ms, 3), "higher_is_better": True,
              "scaling": "strong" if args.total_bytes else "weak", "vs_baseline": None, "dtype": "u8",
              "data": "synthetic" if wname != "enwik8" else "enwik8",
              "config": {"workload": f"level {LEVEL} {wname}, {seg_bytes} bytes per GPU, {total} bytes in one stream, "
                                     "full RLE1->BWT->MTF->Huffman pipeline",
                         "parallelism": f"block-sharded x{world}, single process (bzh_create_multi), devices {devices}"},
              "per_worker_ms": per_worker, "collective_backend": "none: chain by host variables, strings by hipMemcpyPeer",
              "compressed_bytes": out_len}
    if args.full:
        result["checks"] = checks
    print(json.dumps(result), flush=True)
    if not all(checks.values()):
        raise SystemExit("bench: correctness check failed")


def main():
    args = parse_args()
    if args.single_process:
        return single_process(args)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))

    import numpy as np
    import torch
    import torch.distributed as dist
    from banzai_amd import _native as nv
    from banzai_amd import corpus, sharded

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback)")
    # BZH_BENCH_SHARED_GPU=1 (test aid, tests/test_gpu_parity.py): every rank computes on cuda:0 and the collectives run
    # over gloo on host tensors -- the whole multi-rank flow of this script and of sharded.encode_sharded on a box with
    # ONE GPU (RCCL refuses two ranks on one device).  Its numbers are not a measurement of anything.
    shared_gpu = world > 1 and os.environ.get("BZH_BENCH_SHARED_GPU") == "1"
    # BZH_BENCH_DIST_WORLD1=1 (test aid): a single rank takes the MULTI-rank flow -- process group on RCCL (backend "nccl"),
    # gloo side group, broadcast / all_gather / gather / all_reduce on device tensors, encode_sharded -- which is as much
    # of the N > 1 transport as a box with one GPU can execute.  Not a measurement of anything.
    multi = world > 1 or os.environ.get("BZH_BENCH_DIST_WORLD1") == "1"
    if shared_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    cdev = torch.device("cpu") if shared_gpu else dev  # where the tensors of this script's own collectives live
    if multi:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if "MASTER_PORT" not in os.environ:  # (only the one-rank test mode gets here: launchers set it)
            import socket
            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                os.environ["MASTER_PORT"] = str(sk.getsockname()[1])
        if shared_gpu:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    seg_bytes = args.bytes
    total = seg_bytes * world
    if args.total_bytes:
        total = args.total_bytes
        seg_bytes = -(-total // world)
    # ---- workload (untimed): rank k generates segment k; every rank keeps its own range + the look-ahead only ----
    seg_len = max(0, min(seg_bytes, total - rank * seg_bytes))
    seg, wname = corpus.workload(max(1, seg_len), segment=rank)
    seg = seg[:seg_len]
    calib = None
    if multi:
        # how much shorter rank r+1's range is than rank r's follows from what one block costs to CUT (the chain every later
        # rank waits for) against what it costs to ENCODE: rank 0 measures both on the first bytes of the workload, everyone
        # takes its figures (sharded.set_plan_cost), and the line carries the chain's arithmetic per rank beside the clocks
        cal = torch.zeros(3, dtype=torch.float64, device=cdev)
        if rank == 0 and seg_len:
            cn = min(seg_len, 30_000_000)
            d_c = torch.zeros(cn + 16, dtype=torch.uint8, device=dev)
            d_c[:cn] = torch.from_numpy(seg[:cn]).to(dev)
            d_co = torch.zeros((cn + cn // 4 + (1 << 20)) & ~3, dtype=torch.uint8, device=dev)
            with nv.Context(local_rank, LEVEL) as cctx:
                cctx.encode_device(d_c.data_ptr(), cn, d_co.data_ptr(), d_co.numel())  # (first touch)
                best_s = best_e = None
                for _ in range(3):
                    cctx.plan_tables_device(d_c.data_ptr(), cn)
                    torch.cuda.synchronize()
                    tq = time.perf_counter()
                    cctx.plan_split_device(0, None, crc=False)
                    torch.cuda.synchronize()
                    ds = time.perf_counter() - tq
                    nbk = len(cctx.plan_blocks_np())
                    tq = time.perf_counter()
                    cctx.encode_range_device(0, nbk, d_co.data_ptr(), d_co.numel())
                    torch.cuda.synchronize()
                    de = time.perf_counter() - tq
                    best_s = ds if best_s is None or ds < best_s else best_s
                    best_e = de if best_e is None or de < best_e else best_e
                cal[0], cal[1], cal[2] = best_s * 1e3 / nbk, best_e * 1e3 / nbk, cn / nbk
            del d_c, d_co
        dist.broadcast(cal, src=0)
        calib = [float(x) for x in cal.tolist()]
        if calib[1] > 0:
            sharded.set_plan_cost(calib[0], calib[1])
    lo_res, hi_res = sharded.resident_range(total, rank, world) if multi else (0, total)
    resident = hi_res - lo_res
    d_in = torch.zeros(resident + 16, dtype=torch.uint8, device=dev)
    if multi:
        scratch = torch.empty(seg_bytes, dtype=torch.uint8, device=cdev)
        for k in range(world):
            klen = max(0, min(seg_bytes, total - k * seg_bytes))
            if k == rank and klen:
                scratch[:klen].copy_(torch.from_numpy(seg))
            dist.broadcast(scratch, src=k)
            lo, hi = max(k * seg_bytes, lo_res), min(k * seg_bytes + klen, hi_res)
            if hi > lo:
                d_in[lo - lo_res:hi - lo_res] = scratch[lo - k * seg_bytes:hi - k * seg_bytes].to(dev)
        del scratch
    else:
        d_in[:total] = torch.from_numpy(seg).to(dev)
    out_cap = (total // 3 + total // 8 + (1 << 20)) & ~3 if not multi else (total + total // 4 + (1 << 20)) & ~3
    d_out = torch.zeros(out_cap if rank == 0 else 16, dtype=torch.uint8, device=dev)

    ctx = nv.Context(local_rank, LEVEL)  # (the library's default batch: 576 level-9 blocks)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream.cuda_stream)

    engine = None
    side = None
    if multi:
        engine = sharded.DeviceEngine(ctx, d_in, total, d_out, sharded.worst_case_slab(total, world, LEVEL), resident=resident,
                                      lo=lo_res)
        engine.check_lookahead(rank, world)
        side = sharded.side_group(dist)  # the chain's 8-byte hand-offs: gloo, CPU tensors (the collectives stay on RCCL)
        if shared_gpu and os.environ.get("BZH_SHARED_GPU_NO_TURNS") != "1":
            # the ranks take turns on the one GPU (a file lock around every engine call, released once the GPU is idle):
            # the kernels' decoupled look-backs assume the workgroup -> XCD dealing a process sees when it has the device
            # to itself; several processes computing at once perturb it, and a look-back can give up (an error status
            # after a bounded wait, never a hang -- DESIGN.md section 5).  One process per GPU is the deployment.
            import fcntl
            import tempfile
            lock_f = open(os.path.join(tempfile.gettempdir(), f"bzhip_shared_gpu_{os.environ.get('MASTER_PORT', '0')}.lock"), "w")

            def taking_turns(fn):
                def call(*a, **kw):
                    fcntl.flock(lock_f, fcntl.LOCK_EX)
                    try:
                        out = fn(*a, **kw)
                        torch.cuda.synchronize()
                        return out
                    finally:
                        fcntl.flock(lock_f, fcntl.LOCK_UN)
                return call
            for name in ("tables", "split", "encode_range", "assemble"):
                setattr(engine, name, taking_turns(getattr(engine, name)))

    def step():
        """One pass of the hot path; returns the stream length on rank 0."""
        if not multi:
            return ctx.encode_device(d_in.data_ptr(), total, d_out.data_ptr(), out_cap)
        return sharded.encode_sharded(engine, dist, rank, world, side=side)

    def barrier():
        if multi:
            dist.barrier()
        torch.cuda.synchronize()

    out_len = step()  # (first touch: the library sizes and allocates its arena and workspaces inside this call)
    # ---- untimed, FIRST (--full): the same K steps with profiling on (HIP events on the context's stream): stage timings and the
    # per-kernel table -- and the device has reached its clocks by the time the W warm-up steps and the timed region run
    # (a fresh box measured 1-2 % slower when the timed region came first)
    if args.full:
        ctx.set_profiling(True)
        sort_ms = sort_launches = sort_elems = 0.0
        stage, counters = {}, {}
        kern = {}
        rank_ms = {}
        barrier()
        tp0 = time.perf_counter()
        for _ in range(args.steps):
            out_len = step()
            st = ctx.stats()
            if engine is not None:
                for k, v in engine.times.items():
                    rank_ms[k] = rank_ms.get(k, 0.0) + v
            for ks in ctx.kernel_stats():
                acc = kern.setdefault(ks["name"], {"ms": 0.0, "launches": 0, "alg_bytes": 0})
                acc["ms"] += ks["ms"]
                acc["launches"] += ks["launches"]
                acc["alg_bytes"] += ks["alg_bytes"]
            sort_ms += st["ms_bwt_sort"]
            sort_launches += st["bwt_sort_launches"]
            sort_elems += st["bwt_sort_elems"]
            nblocks = st["blocks"]
            for k in ("ms_plan", "ms_rle1", "ms_bwt", "ms_mtf", "ms_huff", "ms_pack"):
                stage[k] = stage.get(k, 0.0) + st[k]
            counters = {k: st[k] for k in ("raw_bytes", "rle_bytes", "bwt_active_sum", "mtf_syms", "out_bits", "bwt_rounds")}
        barrier()
        ms_profiled = (time.perf_counter() - tp0) * 1e3 / args.steps
        ctx.set_profiling(False)

    ctx.set_profiling(False)
    for _ in range(args.warmup):
        out_len = step()
    # ---- timed region: exactly K steps, profiling off, barrier + synchronize on both sides ----
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out_len = step()
    barrier()
    dt = time.perf_counter() - t0
    if multi:
        tmax = torch.tensor([dt], dtype=torch.float64, device=cdev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())
    ms_per_step = dt * 1e3 / args.steps
    value = total * args.steps / dt / 1e6
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, d_out[:out_len].cpu().numpy())
    head = {"metric": METRIC, "value": round(value, 2), "unit": "MB/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3), "higher_is_better": True, "scaling": "strong" if args.total_bytes else "weak",
            "ranks_seen": dist.get_world_size() if multi else 1,
            "chain_calibration": ({"split_ms_per_block": round(calib[0], 5), "encode_ms_per_block": round(calib[1], 5),
                                   "input_bytes_per_block": round(calib[2]), "plan_cost": round(sharded.PLAN_COST, 5)}
                                  if calib and calib[1] > 0 else None),
            "collective_backend": dist.get_backend() if multi else None,
            "vs_baseline": None, "dtype": "u8", "data": "synthetic" if wname != "enwik8" else "enwik8",
            "config": {"workload": f"level {LEVEL} {wname}, {seg_bytes} bytes per GPU, {total} bytes in one stream, "
                                   "full RLE1->BWT->MTF->Huffman pipeline",
                       "parallelism": f"block-sharded x{world}",
                       "input_resident_on_rank0": int(resident)}}
    if not args.full:
        if rank == 0:
            print(json.dumps(dict(head, compressed_bytes=out_len)), flush=True)
        ctx.close()
        if multi:
            dist.barrier()
            dist.destroy_process_group()
        return

    # whole-path accounting needs every rank's counters
    alg = float(path_alg_bytes(counters))
    per_rank = None
    if multi:
        t = torch.tensor([alg], dtype=torch.float64, device=cdev)
        dist.all_reduce(t)
        alg = float(t.item())
        # every rank's share of a step: tables + split, waiting for the chain, encode, gather (+ assembly on rank 0)
        keys = ("ms_plan", "ms_wait", "ms_encode", "ms_gather")
        mine = torch.tensor([rank_ms.get(k, 0.0) / args.steps for k in keys] + [float(resident), float(counters["raw_bytes"])],
                            dtype=torch.float64, device=cdev)
        allr = torch.zeros(world * mine.numel(), dtype=torch.float64, device=cdev)
        dist.all_gather_into_tensor(allr, mine)
        rows = allr.view(world, -1).tolist()
        per_rank = [dict({k: round(v, 3) for k, v in zip(keys, row)}, resident_bytes=int(row[4]), encoded_input_bytes=int(row[5]))
                    for row in rows]
        if calib and calib[1] > 0:  # the chain's arithmetic from rank 0's calibration (sharded.model_finish_ms), beside the clocks
            for row, (mw, msp, men, mfin) in zip(per_rank, sharded.model_finish_ms(total, world, calib[0], calib[1], calib[2])):
                row["model"] = {"wait": round(mw, 3), "split": round(msp, 3), "encode": round(men, 3), "finish": round(mfin, 3)}
        # rank 0 also checks the sharded stream against one GPU encoding the whole input (untimed)
        d_full = torch.zeros(seg_bytes * world + 16, dtype=torch.uint8, device=cdev) if rank == 0 else None
        parts = [d_full[k * seg_bytes:(k + 1) * seg_bytes] for k in range(world)] if rank == 0 else None
        mine_full = torch.zeros(seg_bytes, dtype=torch.uint8, device=cdev)
        mine_full[:seg_len] = torch.from_numpy(seg).to(cdev)
        dist.gather(mine_full, parts, dst=0)
        del mine_full
        if rank == 0:
            d_full = d_full.to(dev)
    else:
        d_full = d_in

    result = None
    if rank == 0:
        stream_bytes = d_out[:out_len].cpu().numpy().tobytes()
        checks = {}
        ref_in = None
        if total <= 200_000_000:
            import bz2
            ref_in = d_full[:total].cpu().numpy().tobytes()
            checks["libbz2_roundtrip"] = bool(bz2.decompress(stream_bytes) == ref_in)
        if multi:
            mcap = (total // 3 + total // 8 + (1 << 20)) & ~3
            d_mono = torch.zeros(mcap, dtype=torch.uint8, device=dev)
            mlen = ctx.encode_device(d_full.data_ptr(), total, d_mono.data_ptr(), mcap)
            checks["sharded_equals_single_gpu"] = bool(mlen == out_len and torch.equal(d_mono[:mlen], d_out[:out_len]))
            del d_mono
        cpu = None
        po = None
        if not args.no_cpu:
            from oracle import pyoracle as po
            sample_n = min(args.cpu_sample, seg_bytes)
            sample = d_full[:sample_n].cpu().numpy()
            t1 = time.perf_counter()
            oracle_stream = po.encode(sample.tobytes(), LEVEL)
            cpu_dt = time.perf_counter() - t1
            d_s_out = torch.zeros((sample_n // 2 + (1 << 20)) & ~3, dtype=torch.uint8, device=dev)
            slen = ctx.encode_device(d_full.data_ptr(), sample_n, d_s_out.data_ptr(), d_s_out.numel())
            checks["bit_exact_vs_oracle_sample"] = bool(d_s_out[:slen].cpu().numpy().tobytes() == oracle_stream)
            del d_s_out
            if ref_in is not None:  # the in-repo strict decoder (oracle/bz2_decode.c) on the whole GPU stream
                try:
                    checks["inrepo_decoder_roundtrip"] = bool(po.decode(stream_bytes, cap=total + 64) == ref_in)
                except po.DecodeError:
                    checks["inrepo_decoder_roundtrip"] = False
            cpu = {"value": round(sample_n / cpu_dt / 1e6, 3), "unit": "MB/s", "cores": 1, "kind": "port",
                   "sample": f"first {sample_n} bytes of the workload, level {LEVEL}, oracle/banzai_oracle.c -O2, "
                             f"1 thread of {os.cpu_count()} host cores"}

        # ---- PCIe-inclusive rate: pinned host buffers through bzh_encode (H2D + encode + D2H inside the clock) ----
        host_incl = None
        stream_api = None
        extras = None
        if not multi and not args.no_extra:
            h_in = torch.from_numpy(seg).pin_memory()
            h_out = torch.zeros(out_cap, dtype=torch.uint8).pin_memory()
            hlen = ctx.encode_host_ptr(h_in.data_ptr(), total, h_out.data_ptr(), out_cap)
            torch.cuda.synchronize()
            th = time.perf_counter()
            for _ in range(args.steps):
                hlen = ctx.encode_host_ptr(h_in.data_ptr(), total, h_out.data_ptr(), out_cap)
            torch.cuda.synchronize()
            hdt = time.perf_counter() - th
            checks["host_path_same_stream"] = bool(h_out[:hlen].numpy().tobytes() == stream_bytes)
            host_incl = {"value": round(total * args.steps / hdt / 1e6, 1), "unit": "MB/s",
                         "ms_per_step": round(hdt * 1e3 / args.steps, 3),
                         "what": "bzh_encode on pinned host buffers: H2D of the input + encode + D2H of the stream inside the clock"}
            del h_in, h_out

            # ---- the reference's API surface: encode(reader, writer, level) = the streaming entry points, fed from
            # PAGEABLE memory in 16 MiB pieces (C ABI: bzh_stream_feed; Python: banzai_amd.encode over BytesIO) ----
            import ctypes
            import io
            import banzai_amd
            FEED = 16 << 20
            sbuf = np.empty(int(nv.lib().bzh_stream_bound(ctx.handle, total)) + (64 << 20), dtype=np.uint8)
            got = ctypes.c_size_t(0)
            best_c = None
            c_same = True
            for it in range(1 + args.steps):
                ts = time.perf_counter()
                ctx.stream_begin()
                parts = []
                for k in range(0, total, FEED):
                    v = seg[k:k + FEED]
                    ctx.check(nv.lib().bzh_stream_feed(ctx.handle, nv.ptr(v), v.size, 0, nv.ptr(sbuf), sbuf.size, ctypes.byref(got)))
                    if it == 0 and got.value:
                        parts.append(sbuf[:got.value].tobytes())
                ctx.check(nv.lib().bzh_stream_feed(ctx.handle, nv.ptr(sbuf), 0, 1, nv.ptr(sbuf), sbuf.size, ctypes.byref(got)))
                if it == 0:
                    parts.append(sbuf[:got.value].tobytes())
                    c_same = b"".join(parts) == stream_bytes
                else:
                    dts = time.perf_counter() - ts
                    best_c = dts if best_c is None or dts < best_c else best_c
            raw_in = seg.tobytes()
            best_p = None
            p_same = True
            for it in range(3):
                sink = io.BytesIO()
                ts = time.perf_counter()
                banzai_amd.encode(io.BytesIO(raw_in), sink, LEVEL)
                dts = time.perf_counter() - ts
                if it == 0:
                    p_same = sink.getvalue() == stream_bytes
                else:
                    best_p = dts if best_p is None or dts < best_p else best_p
            del raw_in, sbuf
            checks["stream_api_same_stream"] = bool(c_same and p_same)
            stream_api = {"value": round(total / best_c / 1e6, 1), "unit": "MB/s", "ms": round(best_c * 1e3, 2),
                          "python_encode": round(total / best_p / 1e6, 1), "python_ms": round(best_p * 1e3, 2),
                          "feed_bytes": FEED, "frac_of_value": round(total / best_c / 1e6 / value, 3),
                          "what": "bzh_stream_begin/feed from pageable host memory, whole stream back in host memory "
                                  "(best of the timed steps); python_encode = banzai_amd.encode(BytesIO, BytesIO, 9)"}

            # ---- other inputs, each one whole stream on this GPU, bit-exact vs the oracle ----
            extras = {}
            # BASELINE.json configs[1]: ONE 899,999-byte block of uniform-random bytes (xorshift64*): a latency case --
            # one block cannot fill 256 CUs; `ms_bwt` of its record is the "BWT radix-sort kernel only" figure
            sets = [("c2-one-random-block", corpus.xorshift_bytes(899_999))]
            if wname != "enwik8-synthetic":  # rounds 1-3 quoted their headline on this generator
                sets.append(("enwik8-synthetic-v1", corpus.enwik_synthetic(100_000_000)))
            sets += [(name, corpus.image_corpus(name)) for name in corpus.IMAGE_SETS] + corpus.c5_parts(100_000_000)
            # the oracle's streams of all of them on a thread pool (ctypes releases the GIL): the CPU legs used to be
            # 90 % of this script's wall time, one after the other on one core
            pool = None
            futs = {}
            if po is not None:
                from concurrent.futures import ThreadPoolExecutor
                pool = ThreadPoolExecutor(max_workers=max(1, min(len(sets), (os.cpu_count() or 2) - 1)))

                def oracle_leg(buf):
                    tc = time.perf_counter()
                    w = po.encode(buf, LEVEL)
                    return w, time.perf_counter() - tc
                for name, data in sets:
                    if int(data.size) >= 500_000:
                        futs[name] = pool.submit(oracle_leg, data.tobytes())
            for name, data in sets:
                n = int(data.size)
                if n < 500_000:
                    extras[name] = {"skipped": f"only {n} bytes found"}
                    continue
                d_x = torch.zeros(n + 16, dtype=torch.uint8, device=dev)
                d_x[:n] = torch.from_numpy(np.array(data, dtype=np.uint8, copy=True)).to(dev)
                xcap = (n + n // 4 + (1 << 20)) & ~3
                d_y = torch.zeros(xcap, dtype=torch.uint8, device=dev)
                ctx.set_profiling(False)
                xlen = ctx.encode_device(d_x.data_ptr(), n, d_y.data_ptr(), xcap)  # warm-up
                best = None
                for _ in range(3):
                    torch.cuda.synchronize()
                    tx = time.perf_counter()
                    xlen = ctx.encode_device(d_x.data_ptr(), n, d_y.data_ptr(), xcap)
                    torch.cuda.synchronize()
                    dx = time.perf_counter() - tx
                    best = dx if best is None or dx < best else best
                ctx.set_profiling(True)
                ctx.encode_device(d_x.data_ptr(), n, d_y.data_ptr(), xcap)
                xs = ctx.stats()
                ctx.set_profiling(False)
                rec = {"bytes": n, "MB/s": round(n / best / 1e6, 1), "ms": round(best * 1e3, 2),
                       "ms_bwt": round(xs["ms_bwt"], 3), "ms_mtf": round(xs["ms_mtf"], 3),
                       "rounds": int(xs["bwt_rounds"]), "A/n": round(xs["bwt_active_sum"] / max(1, xs["rle_bytes"]), 2),
                       "ratio": round(xlen / n, 4)}
                if name in corpus.IMAGE_SETS:  # whatever files this image holds: say exactly which bytes were measured
                    rec["sha256"] = corpus.corpus_digest(data)
                    rec["files"] = int(corpus.LAST_FILE_COUNT.get(name, 0))
                rec["_stream"] = d_y[:xlen].cpu().numpy().tobytes()
                extras[name] = rec
                del d_x, d_y
            for name, rec in extras.items():
                got_stream = rec.pop("_stream", None)
                if name in futs:
                    want, odt = futs[name].result()
                    rec["oracle_MB/s"] = round(rec["bytes"] / odt / 1e6, 1)
                    rec["oracle_threads"] = "one per workload, all workloads at once"
                    rec["bit_exact"] = bool(got_stream == want)
                    checks[f"bit_exact_{name}"] = rec["bit_exact"]
            if pool is not None:
                pool.shutdown()

            def timed_encode(c, d_x, n, d_y, xcap, reps=3):
                xlen = c.encode_device(d_x.data_ptr(), n, d_y.data_ptr(), xcap)  # warm-up (and first touch of a grown arena)
                best = None
                for _ in range(reps):
                    torch.cuda.synchronize()
                    tx = time.perf_counter()
                    xlen = c.encode_device(d_x.data_ptr(), n, d_y.data_ptr(), xcap)
                    torch.cuda.synchronize()
                    dx = time.perf_counter() - tx
                    best = dx if best is None or dx < best else best
                return xlen, best

            # ---- how the headline depends on the stand-in: the v2 generator at 3 % (the calibrated headline), 6 % and 12 %
            # copied bytes -- the share of verbatim repeats sets the depth of the suffix sort (rounds, A/n), the compression
            # ratio barely moves
            sensitivity = []
            if wname == "enwik8-synthetic-v2":
                for frac in (0.03, 0.06, 0.12):
                    data = seg if frac == 0.03 else corpus.enwik_synthetic_v2(total, repeat_fraction=frac)
                    d_x = torch.zeros(total + 16, dtype=torch.uint8, device=dev)
                    d_x[:total] = torch.from_numpy(data).to(dev)
                    d_y = torch.zeros(out_cap, dtype=torch.uint8, device=dev)
                    xlen, best = timed_encode(ctx, d_x, total, d_y, out_cap)
                    ctx.set_profiling(True)
                    ctx.encode_device(d_x.data_ptr(), total, d_y.data_ptr(), out_cap)
                    xs = ctx.stats()
                    ctx.set_profiling(False)
                    sensitivity.append({"copied_fraction": frac, "MB/s": round(total / best / 1e6, 1), "ms": round(best * 1e3, 2),
                                        "rounds": int(xs["bwt_rounds"]), "A/n": round(xs["bwt_active_sum"] / max(1, xs["rle_bytes"]), 3),
                                        "ratio": round(xlen / total, 4)})
                    del d_x, d_y

            # ---- streams of more than one batch on ONE GPU (BASELINE config 4 and the shape of one of its eight ranks): the
            # library's default batch (576 blocks) against batches of 128 blocks, one lane against two; every variant must give
            # the bytes of the first, the 125 MB stream also goes through the in-repo strict decoder
            multibatch = {}
            if total == SEGMENT:
                big = np.concatenate([seg] + [corpus.workload(SEGMENT, segment=k)[0] for k in range(1, 10)])
                for name, n in (("c4-rank-shape-125MB", 125_000_000), ("c4-1GB-one-gpu", 1_000_000_000)):
                    d_x = torch.zeros(n + 16, dtype=torch.uint8, device=dev)
                    d_x[:n] = torch.from_numpy(big[:n]).to(dev)
                    xcap = (n // 3 + n // 8 + (1 << 20)) & ~3
                    d_y = torch.zeros(xcap, dtype=torch.uint8, device=dev)
                    rec = {"bytes": n, "variants": []}
                    ref = None
                    same = True
                    for mb, lanes in ((0, 1), (128, 1), (128, 2), (0, 2)):
                        with nv.Context(local_rank, LEVEL, mb) as c2:
                            c2.set_lanes(lanes)
                            xlen, best = timed_encode(c2, d_x, n, d_y, xcap, reps=2)
                            blocks = int(c2.stats()["blocks"])
                        got = d_y[:xlen].clone()
                        if ref is None:
                            ref = got
                        same = same and bool(got.numel() == ref.numel() and torch.equal(got, ref))
                        rec["variants"].append({"max_batch": mb or "default (576)", "lanes": lanes, "MB/s": round(n / best / 1e6, 1),
                                                "ms": round(best * 1e3, 2)})
                        del got
                    rec["blocks"] = blocks
                    rec["MB/s"] = rec["variants"][0]["MB/s"]
                    rec["all_variants_same_stream"] = same
                    checks[f"same_stream_all_batchings_{name}"] = same
                    if po is not None and n <= 200_000_000:
                        try:
                            rec["inrepo_decoder_roundtrip"] = bool(po.decode(ref.cpu().numpy().tobytes(), cap=n + 64) == big[:n].tobytes())
                        except po.DecodeError:
                            rec["inrepo_decoder_roundtrip"] = False
                        checks[f"inrepo_decoder_{name}"] = rec["inrepo_decoder_roundtrip"]
                    multibatch[name] = rec
                    del d_x, d_y, ref
                del big
                extras.update(multibatch)

        # every radix_scatter launch together (the figure rounds 1-3 quoted as the dominant kernel): algorithmic bytes /
        # HIP-event time
        achieved_rs = (SORT_BYTES_PER_ELEM * sort_elems / (sort_ms * 1e-3) / 1e9) if sort_ms > 0 else None
        # per-kernel-class roofline: HIP-event time of the class's launches in the profiled pass, algorithmic bytes
        # by DESIGN.md section 4's per-element figures; the six classes that took the most time
        ktable = []
        for name, v in sorted(kern.items(), key=lambda kv: -kv[1]["ms"]):
            if v["ms"] <= 0:
                continue
            gbs = v["alg_bytes"] / (v["ms"] * 1e-3) / 1e9 if v["alg_bytes"] else None
            ktable.append({"kernel": name, "us_per_step": round(v["ms"] * 1e3 / args.steps, 1),
                           "launches_per_step": round(v["launches"] / args.steps, 1),
                           "alg_bytes_per_step": round(v["alg_bytes"] / args.steps),
                           "achieved_GBs": round(gbs, 1) if gbs else None,
                           "frac": round(gbs / HBM_PEAK_GBS, 4) if gbs else None})
        # the DOMINANT kernel class = the one that took the most time in the profiled pass.  Since the bucket-first initial
        # sort is the default for text that is chunk_finish -- one launch per step that sorts every bucket inside LDS; its
        # algorithmic HBM bytes are 8 in + 8 out per suffix + 8 per list record, its bound is LDS / issue, not HBM (the
        # point of it: the passes it replaces moved 8x the bytes) -- so `frac` against the HBM peak is small by design.
        # HBM bytes per launch from the committed PMC passes of this same command (FETCH_SIZE / WRITE_SIZE in separate
        # rocprofv3 runs, corrected as MI355X_MICROARCH.md prescribes); null if not collected
        dom = ktable[0] if ktable else None
        dom_launches = dom["launches_per_step"] if dom else 0
        dom_us = (dom["us_per_step"] / dom_launches) if dom and dom_launches else None
        dom_bytes = (dom["alg_bytes_per_step"] / dom_launches) if dom and dom_launches else None
        dom_key = dom["kernel"].split(" ")[0].split("<")[0] if dom else ""
        traffic = None
        traffic_source = None
        try:
            pmc = sorted(p for p in os.listdir(os.path.join(ROOT, "profiles")) if p.endswith("_pmc_traffic.json"))
            if pmc and not multi and seg_bytes == SEGMENT and dom_key:
                with open(os.path.join(ROOT, "profiles", pmc[-1])) as f:
                    pk = json.load(f)["kernels"]
                hit = [v for k, v in pk.items() if k.startswith(dom_key)]
                nl = sum(v["launches"] for v in hit)
                if nl:
                    traffic = round(sum(v["hbm_bytes_per_launch"] * v["launches"] for v in hit) / nl)
                    traffic_source = (f"profiles/{pmc[-1]}: separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE runs of this "
                                      f"command (kernels named {dom_key}*), NOT measured in this run")
        except Exception:
            traffic = None
        # all kernels' HBM bytes of one step by the counters (the same committed PMC passes: launches x bytes per launch over
        # the file's steps) against the timed step: how busy HBM is, whatever the fixed accounting of `path_frac` says
        hbm_util = None
        try:
            if pmc and not multi and seg_bytes == SEGMENT:
                with open(os.path.join(ROOT, "profiles", pmc[-1])) as f:
                    pj = json.load(f)
                psteps = float(pj.get("steps_in_run", 0) or 0)
                if psteps > 0:
                    pbytes = sum(v["hbm_bytes_per_launch"] * v["launches"] for v in pj["kernels"].values()) / psteps
                    hbm_util = {"bytes_per_step": round(pbytes), "frac": round(pbytes / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                "source": f"profiles/{pmc[-1]} (all kernels, FETCH_SIZE with the gfx950 correction + WRITE_SIZE) over this run's ms_per_step"}
        except Exception:
            hbm_util = None
        ktable = ktable[:10]
        path_gbs = alg / (ms_per_step * 1e-3) / 1e9
        v_range = [v for v in (value, (extras or {}).get("enwik8-synthetic-v1", {}).get("MB/s"),
                               (extras or {}).get("real-text-100MB", {}).get("MB/s")) if v]
        result = {
            **head, "per_rank": per_rank,
            "config": dict(head["config"], blocks_on_rank0=int(nblocks)),
            # text-like 100 MB inputs span this range on one MI355X: the calibrated stand-in, the rounds 1-3 generator, real text
            # of the image (the stand-in is the EASIEST of the three for the suffix sort: see `sensitivity`)
            "value_range": {"min": round(min(v_range), 1), "max": round(max(v_range), 1),
                            "over": "headline (enwik8-synthetic-v2), enwik8-synthetic-v1, real-text-100MB"} if len(v_range) == 3 else None,
            "sensitivity": sensitivity if (not multi and not args.no_extra) else None,
            "roofline": {"bound": ("lds/issue" if dom_key in ("chunk_finish", "mid_sort", "mtf_walk") else "hbm"),
                         "bound_note": "what limits the dominant kernel; `peak`, `achieved` and `frac` are still HBM figures "
                                       "(algorithmic bytes over launch time against 8 TB/s), as the contract defines them",
                         "hbm_util_counters": hbm_util,
                         "kernel": dom["kernel"] if dom else None,
                         "achieved": dom["achieved_GBs"] if dom else None,
                         "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": dom["frac"] if dom else None, "traffic": traffic,
                         "traffic_source": traffic_source, "kernels": ktable,
                         "launches": int(round(dom_launches * args.steps)) if dom else 0,
                         "avg_launch_us": round(dom_us, 2) if dom_us else None,
                         "alg_bytes_per_launch": round(dom_bytes) if dom_bytes else None,
                         "limited_by": "LDS / instruction issue (an in-LDS sort: HBM sees one read and one write of every "
                                       "suffix)" if dom_key == "chunk_finish" else None,
                         "radix_scatter_all": {"achieved": round(achieved_rs, 1) if achieved_rs else None,
                                               "frac": round(achieved_rs / HBM_PEAK_GBS, 4) if achieved_rs else None,
                                               "launches": int(sort_launches),
                                               "avg_launch_us": round(sort_ms * 1e3 / sort_launches, 2) if sort_launches else None},
                         "measured_in": "untimed pass of the same K steps with profiling on, before the warm-up and the timed region "
                                        f"({round(ms_profiled, 3)} ms per step there)",
                         # the whole path by SURVEY 8(d)'s fixed accounting, over the TIMED region (all ranks)
                         "path_alg_bytes_per_step": round(alg), "path_achieved": round(path_gbs, 1),
                         "path_frac": round(path_gbs / (HBM_PEAK_GBS * world), 4),
                         "path_A_convention": "A = unresolved suffixes entering each doubling round actually run.  A block on the "
                                              "bucket-first initial sort enters round 0 at depth 7; the round-0 step of its small "
                                              "groups (8 text bytes per member, ranked in LDS) runs inside chunk_finish and its "
                                              "members count for round 0 as they would in a kernel of their own; a block on the "
                                              "8 passes enters at depth 8"},
            "cpu_baseline": cpu,
            "value_host_inclusive": host_incl,
            "value_stream_api": stream_api,
            "value_real_text": (extras or {}).get("real-text-100MB", {}).get("MB/s"),
            # the generator rounds 1-3 quoted their headline on (driver lines on it: r1 6,344, r2 7,146, r3 8,858; r4 measured 8,977 on it in `extra_workloads`):
            # the same-input series across rounds
            "value_v1": (extras or {}).get("enwik8-synthetic-v1", {}).get("MB/s"),
            "workload_sha256": corpus.corpus_digest(seg) if not multi else None,
            # north_star's ">= 10x banzai's CPU path, one thread": quoted on the LOWER of the headline and the real-text
            # workload (GPU MB/s over the oracle's MB/s on the same bytes)
            "speedup_vs_cpu_1thread": (lambda rt: {
                "headline": round(value / cpu["value"], 1) if cpu else None,
                "real_text": round(rt["MB/s"] / rt["oracle_MB/s"], 1) if rt.get("oracle_MB/s") else None,
            })((extras or {}).get("real-text-100MB", {})),
            "stage_ms_per_step": {k: round(v / args.steps, 3) for k, v in stage.items()},
            "bwt_rounds": int(counters.get("bwt_rounds", 0)),
            "A_over_n": round(counters["bwt_active_sum"] / max(1, counters["rle_bytes"]), 3),
            "extra_workloads": extras,
            "compressed_bytes": out_len, "checks": checks,
        }
        print(json.dumps(result), flush=True)
    ctx.close()
    if multi:
        dist.barrier()
        dist.destroy_process_group()
    if result is not None and not all(result["checks"].values()):
        raise SystemExit("bench: correctness check failed")


if __name__ == "__main__":
    main()
