// api.hip -- the C ABI of libbzhip.so (include/bzhip.h): context, workspace, whole-path drivers
// and the host-pointer stage seams used by the parity tests.
//
// Whole path = the loop of banzai::encode (reference lib/lib.rs:84-132) turned inside out:
//   plan    : RLE1 run scan + every block cut + block CRCs            (rle1.hip)
//   batches : RLE1 emit -> BWT -> MTF/RLE2 -> Huffman tables + bit lengths (all blocks at once)
//   pack    : block headers + payload bits written straight at their final bit offset
//   assemble: "BZh9", stream CRC fold, footer
#include <stdarg.h>
#include <algorithm>
#include <atomic>
#include <future>
#include <mutex>
#include <new>
#include <thread>

#include "common.h"
#include "decode_plan.h"
#include "decode_records_plan.h"
#include "decode_recover_plan.h"
#include "encode_plan.h"
#include "grep_many_plan.h"
#include "recover_gather.h"
#include "stream_index.h"

static void stream_join(bzh_ctx *ctx); // waits for a streaming pass in flight (defined with bzh_stream_*)

// The error text has two writers while a streaming pass is in flight (the caller's thread and the pass's
// worker thread), so it is guarded; readers get a private copy (bzh_last_error).
void bzh_set_error(bzh_ctx *ctx, const char *fmt, ...)
{
    if (!ctx) return;
    std::lock_guard<std::mutex> g(ctx->err_mu);
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(ctx->err, sizeof ctx->err, fmt, ap);
    va_end(ap);
}

// Nothing unwinds across the C ABI (include/bzhip.h): every entry point runs inside this guard.  The
// reference's convention is the same -- errors are values (io::Result, lib/lib.rs:84-92), panics never
// cross the boundary.
template <typename F>
static int bzh_guard(bzh_ctx *ctx, F &&body) noexcept
{
    try {
        return body();
    } catch (const std::bad_alloc &) {
        bzh_set_error(ctx, "host allocation failed");
        return BZH_E_NOMEM;
    } catch (const std::exception &e) {
        bzh_set_error(ctx, "internal error: %s", e.what());
        return BZH_E_STATE;
    } catch (...) {
        bzh_set_error(ctx, "internal error");
        return BZH_E_STATE;
    }
}

// Only gfx950 code objects are in the library: "gfx950", optionally followed by feature flags
// (hipDeviceProp_t::gcnArchName reads e.g. "gfx950:sramecc+:xnack-").
extern "C" int bzh_arch_supported(const char *gcn_arch_name)
{
    if (!gcn_arch_name) return 0;
    if (strncmp(gcn_arch_name, "gfx950", 6) != 0) return 0;
    return gcn_arch_name[6] == 0 || gcn_arch_name[6] == ':';
}

hipEvent_t bzh_event(bzh_ctx *ctx)
{
    if (ctx->evnext == ctx->evpool.size()) {
        hipEvent_t e;
        hipEventCreate(&e);
        ctx->evpool.push_back(e);
    }
    return ctx->evpool[ctx->evnext++];
}

// Profiling: an event of the pool recorded on the context's stream now (nullptr otherwise).
static hipEvent_t call_mark(bzh_ctx *ctx)
{
    if (!ctx->profiling) return nullptr;
    hipEvent_t e = bzh_event(ctx);
    hipEventRecord(e, ctx->stream);
    return e;
}

extern "C" const char *bzh_strerror(int status)
{
    switch (status) {
    case BZH_OK: return "ok";
    case BZH_E_ARG: return "invalid argument";
    case BZH_E_NOMEM: return "out of memory";
    case BZH_E_HIP: return "HIP runtime error or no usable gfx950 device";
    case BZH_E_CAP: return "output buffer too small";
    case BZH_E_STATE: return "call sequence error";
    case BZH_E_DATA: return "not a valid bzip2 stream";
    default: return "unknown status";
    }
}

extern "C" const char *bzh_last_error(const bzh_ctx *cctx)
{
    if (!cctx) return "no context";
    bzh_ctx *ctx = const_cast<bzh_ctx *>(cctx);
    std::lock_guard<std::mutex> g(ctx->err_mu);
    memcpy(ctx->err_out, ctx->err, sizeof ctx->err_out);
    return ctx->err_out;
}

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// The context's second stream with its events (the suffix sort's big-list path, the plan's CRCs), created on first use.
hipStream_t bzh_side_stream(bzh_ctx *ctx)
{
    if (ctx->side_stream) return ctx->side_stream;
    hipStream_t s = nullptr;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int k = 0; k < 4; k++) {
        if (hipEventCreateWithFlags(&ev[k], hipEventDisableTiming) != hipSuccess) {
            for (int j = 0; j < k; j++) hipEventDestroy(ev[j]);
            hipStreamDestroy(s);
            return nullptr;
        }
    }
    ctx->side_ev[0] = ev[0];
    ctx->side_ev[1] = ev[1];
    ctx->plan_ev[0] = ev[2];
    ctx->plan_ev[1] = ev[3];
    ctx->side_stream = s;
    return s;
}

// Makes the arena hold batches of `blocks` blocks (at most max_batch).  It only ever grows: to the size asked for,
// rounded up so that a stream of growing batches does not reallocate every time.  Nothing is in flight on the
// arena when this is called (every entry point waits for its own work before it returns).
static int ensure_arena(bzh_ctx *ctx, uint32_t blocks, size_t min_bytes = 0)
{
    blocks = std::max<uint32_t>(1, std::min<uint32_t>(blocks, ctx->max_batch));
    if (ctx->arena && blocks <= ctx->arena_blocks && min_bytes <= ctx->arena.cap) return BZH_OK;
    const uint32_t want = arena_batch(blocks, ctx->max_batch);
    Batch probe{};
    const char *misfit = nullptr;
    const size_t bytes = std::max(layout_batch(probe, nullptr, want, ctx->M, &misfit), min_bytes);
    if (misfit) {
        bzh_set_error(ctx, "a %u-block workspace at level %d has no room for %s (batch_views)", want, ctx->level, misfit);
        return BZH_E_STATE;
    }
    ctx->arena_blocks = 0;
    BZH_TRY(ctx->arena.reserve(ctx, bytes, "the batch workspace"));
    ctx->arena_blocks = want;
    layout_batch(ctx->bt, ctx->arena, want, ctx->M);
    return BZH_OK;
}

// The context's (or a lane's) pinned readback area, cleared: no stale sequence words.
static int pinned_alloc(bzh_ctx *c)
{
    c->h_pinned.flags = hipHostMallocCoherent;
    BZH_TRY(c->h_pinned.reserve(c, pinned_words(c->max_batch) * sizeof(uint32_t), "the readback area"));
    memset(c->h_pinned, 0, c->h_pinned.cap);
    return BZH_OK;
}

extern "C" int bzh_create(bzh_ctx **out, int device, int level, int max_batch)
{
    return bzh_guard(nullptr, [&]() -> int {
    if (!out || level < 1 || level > 9 || max_batch < 0) return BZH_E_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) return BZH_E_HIP;
    if (hipSetDevice(device) != hipSuccess) return BZH_E_HIP;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess || !bzh_arch_supported(prop.gcnArchName)) return BZH_E_HIP;
    bzh_ctx *ctx = new (std::nothrow) bzh_ctx();
    if (!ctx) return BZH_E_NOMEM;
    ctx->device = device;
    ctx->level = level;
    ctx->M = 100000u * (uint32_t)level - 1u; // lib/rle.rs:121
    // default: a batch covers about 520 MB of RLE1 output at level 9 (576 blocks; 1,024 blocks from level 5 down).  A pass
    // costs about half a millisecond of latency chains whatever its size (the plan, the late doubling rounds, the Huffman
    // heaps), so a long stream is cheaper in few, large batches -- 1 GB on one MI355X: 87.8 ms in batches of 128 blocks,
    // 81.6 ms in 256s, 78.2 ms in 576s (profiles/r06_multibatch.txt).  The arena is sized for the batch actually planned
    // (ensure_arena: 56 MB a block), so only an input that fills such a batch pays for it: 32 GB of 288 GB.
    ctx->max_batch = max_batch ? (uint32_t)max_batch : std::min<uint32_t>(1024u, 576u * 9u / (uint32_t)level);
    // a streaming pass is worth launching once a full batch of input is pending
    ctx->strm.min_feed = std::min<size_t>((size_t)128 << 20, (size_t)ctx->max_batch * (ctx->M + 1));
    Batch probe{};
    (void)layout_batch(probe, nullptr, 1, ctx->M);
    if (probe.TPB > 1024 || ctx->max_batch > 1024) {
        delete ctx;
        return BZH_E_ARG;
    }
    // The workspace arena (about 56 MB per block of a batch, 6.3 GB for the 112 blocks of a 100 MB input) is NOT allocated here:
    // ensure_arena sizes it for the batches actually planned, so a 1 MB file does not pay for a 128-block arena.
    ctx->S = probe.S;
    ctx->bt.S = probe.S;
    ctx->bt.TPB = probe.TPB;
    ctx->bt.M = ctx->M;
    if (pinned_alloc(ctx) != BZH_OK) {
        delete ctx;
        return BZH_E_NOMEM;
    }
    *out = ctx;
    return BZH_OK;
    });
}

extern "C" void bzh_destroy(bzh_ctx *ctx)
{
    if (!ctx) return;
    // a streaming pass in flight keeps launching kernels on the arena and the staging buffers: it ends
    // first, then the device drains, and only then is anything freed
    try {
        if (ctx->strm.worker.joinable()) ctx->strm.worker.join();
    } catch (...) {
    }
    hipSetDevice(ctx->device);
    // only this context's work has to end (other contexts of the device keep running): its stream, the lanes'
    // streams, the streaming copy stream
    hipStreamSynchronize(ctx->stream);
    for (bzh_ctx *l : ctx->lanes)
        if (l->stream) hipStreamSynchronize(l->stream);
    if (ctx->strm.copy_stream) hipStreamSynchronize(ctx->strm.copy_stream);
    auto drop_side = [](bzh_ctx *c) {
        if (!c->side_stream) return;
        hipStreamSynchronize(c->side_stream);
        hipEventDestroy(c->side_ev[0]);
        hipEventDestroy(c->side_ev[1]);
        hipEventDestroy(c->plan_ev[0]);
        hipEventDestroy(c->plan_ev[1]);
        hipStreamDestroy(c->side_stream);
        c->side_stream = nullptr;
        if (c->side2_stream) {
            hipStreamSynchronize(c->side2_stream);
            hipEventDestroy(c->side_ev[2]);
            hipStreamDestroy(c->side2_stream);
            c->side2_stream = nullptr;
        }
    };
    drop_side(ctx);
    for (bzh_ctx *l : ctx->lanes) drop_side(l);
    for (hipEvent_t e : ctx->evpool) hipEventDestroy(e);
    for (bzh_ctx *l : ctx->lanes) {
        for (hipEvent_t e : l->evpool) hipEventDestroy(e);
        if (l->stream) hipStreamDestroy(l->stream);
        delete l;
    }
    if (ctx->strm.copy_stream) hipStreamDestroy(ctx->strm.copy_stream);
    dstream_free(ctx);
    delete ctx; // (its buffers with it: GrowBuf, common.h)
}

extern "C" int bzh_set_stream(bzh_ctx *ctx, void *hip_stream)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx) return BZH_E_ARG;
    ctx->stream = (hipStream_t)hip_stream;
    return BZH_OK;
    });
}

extern "C" int bzh_set_lanes(bzh_ctx *ctx, int lanes)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || (lanes != 1 && lanes != 2)) return BZH_E_ARG;
    ctx->nlanes = lanes;
    return BZH_OK;
    });
}

extern "C" int bzh_set_mode(bzh_ctx *ctx, int mode)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || (mode != BZH_MODE_REFERENCE && mode != BZH_MODE_FIXED)) return BZH_E_ARG;
    ctx->mode = mode;
    for (bzh_ctx *l : ctx->lanes) l->mode = mode;
    return BZH_OK;
    });
}

extern "C" int bzh_set_profiling(bzh_ctx *ctx, int enabled)
{
    return bzh_guard(ctx, [&]() -> int {
    if (!ctx) return BZH_E_ARG;
    ctx->profiling = enabled ? 1 : 0;
    return BZH_OK;
    });
}

extern "C" int bzh_debug_fault(bzh_ctx *ctx, int kind)
{
    return bzh_guard(ctx, [&]() -> int {
    if (!ctx || kind < 0 || kind > 2) return BZH_E_ARG;
    ctx->debug_fault = (uint32_t)kind;
    return BZH_OK;
    });
}

// what every bzh_get_*_stats call does: a copy of one block of the context's statistics
template <typename T>
static int stats_get(const bzh_ctx *ctx, T bzh_ctx::*block, T *out)
{
    return bzh_guard(const_cast<bzh_ctx *>(ctx), [&]() -> int {
    if (!ctx || !out) return BZH_E_ARG;
    *out = ctx->*block;
    return BZH_OK;
    });
}

extern "C" int bzh_get_stats(const bzh_ctx *ctx, bzh_stats *out) { return stats_get(ctx, &bzh_ctx::stats, out); }

static void kstats_reset(bzh_ctx *ctx, bool keep_plan = false) // (keep_plan: the plan's classes stay in the table)
{
    ctx->kspans.clear();
    for (int k = 0; k < K_COUNT; k++) {
        if (keep_plan && (k == K_PLAN || k == K_CRC)) continue;
        ctx->k_ms[k] = 0;
        ctx->k_bytes[k] = 0;
        ctx->k_launch[k] = 0;
    }
}

// Event pairs -> milliseconds per kernel class (the stream has been waited for).
static void kstats_collect(bzh_ctx *ctx)
{
    for (auto &r : ctx->kspans) {
        float t = 0;
        if (hipEventElapsedTime(&t, r.a, r.b) == hipSuccess) ctx->k_ms[r.cls] += t;
    }
    ctx->kspans.clear();
}

// The start of every call that counts or times: fresh statistics and kernel classes, the event pool rewound (every such call
// takes its events from the start of the pool), no span recorded against the old use of those events.
// (`keep_plan`: bzh_encode_range_device -- the plan calls in front of it belong to the same encode: ms_plan stays, and so do the
// plan's kernel classes, whose spans are turned into milliseconds now, before the pool is rewound under them)
static int stats_begin(bzh_ctx *ctx, bool keep_plan = false)
{
    const double ms_plan = keep_plan ? ctx->stats.ms_plan : 0;
    memset(&ctx->stats, 0, sizeof ctx->stats);
    ctx->stats.ms_plan = ms_plan;
    ctx->sort_spans.clear();
    if (keep_plan && ctx->profiling) {
        HIP_TRY(ctx, bzh_stream_wait(ctx->stream));
        kstats_collect(ctx);
    }
    kstats_reset(ctx, keep_plan && ctx->profiling);
    ctx->evnext = 0;
    return BZH_OK;
}

extern "C" int bzh_get_kernel_stats(const bzh_ctx *ctx, bzh_kstat *out, size_t max, size_t *count)
{
    return bzh_guard(const_cast<bzh_ctx *>(ctx), [&]() -> int {
    if (!ctx || !count || (max && !out)) return BZH_E_ARG;
    *count = K_COUNT;
    if (max < (size_t)K_COUNT) return BZH_E_CAP;
    for (int k = 0; k < K_COUNT; k++) {
        memset(&out[k], 0, sizeof out[k]);
        strncpy(out[k].name, KCLASS_NAME[k], sizeof out[k].name - 1);
        out[k].ms = ctx->k_ms[k];
        out[k].launches = ctx->k_launch[k];
        out[k].alg_bytes = ctx->k_bytes[k];
    }
    return BZH_OK;
    });
}

static void stats_collect_sort(bzh_ctx *ctx)
{
    kstats_collect(ctx);
    double ms = 0;
    for (auto &sp : ctx->sort_spans) {
        float t = 0;
        if (hipEventElapsedTime(&t, sp.first, sp.second) == hipSuccess) ms += t;
    }
    ctx->stats.ms_bwt_sort = ms;
}

static int ensure_stage(bzh_ctx *ctx, DevBuf &buf, size_t need) { return buf.reserve(ctx, need, "a staging buffer", grow_eighth); }

// ---- stage seam: BWT ---------------------------------------------------------------------------------
extern "C" int bzh_bwt_batch(bzh_ctx *ctx, const uint8_t *in, const uint64_t *offs, const uint32_t *lens,
                             size_t nblk, uint8_t *bwt_out, uint32_t *ptr, uint8_t *has_byte)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || !in || !offs || !lens || !bwt_out || !ptr || !has_byte) return BZH_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    stats_begin(ctx);
    BZH_TRY(ensure_arena(ctx, (uint32_t)std::min<size_t>(nblk, ctx->max_batch)));
    Batch &bt = ctx->bt;
    for (size_t k0 = 0; k0 < nblk; k0 += ctx->max_batch) {
        uint32_t B = (uint32_t)std::min<size_t>(ctx->max_batch, nblk - k0);
        uint32_t nmax = 0;
        uint64_t ntotal = 0;
        for (uint32_t b = 0; b < B; b++) {
            uint32_t n = lens[k0 + b];
            ntotal += n;
            if (n == 0 || n > ctx->M) {
                bzh_set_error(ctx, "block %zu length %u outside 1..%u", k0 + b, n, ctx->M);
                return BZH_E_ARG;
            }
            nmax = std::max(nmax, n);
            HIP_TRY(ctx, hipMemcpyAsync(bt.rle + (size_t)b * bt.S, in + offs[k0 + b], n, hipMemcpyHostToDevice,
                                        ctx->stream));
        }
        HIP_TRY(ctx, hipMemcpyAsync(bt.n, lens + k0, B * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        BZH_TRY(bwt_run(ctx, B, nmax, ntotal));
        for (uint32_t b = 0; b < B; b++)
            HIP_TRY(ctx, hipMemcpyAsync(bwt_out + offs[k0 + b], bt.bwt + (size_t)b * bt.S, lens[k0 + b],
                                        hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(ptr + k0, bt.ptr, B * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(has_byte + k0 * 256, bt.hasbyte, (size_t)B * 256, hipMemcpyDeviceToHost,
                                    ctx->stream));
        HIP_TRY(ctx, bzh_stream_wait(ctx->stream));
    }
    if (ctx->profiling) stats_collect_sort(ctx);
    return BZH_OK;
    });
}

extern "C" int bzh_bwt(bzh_ctx *ctx, const uint8_t *in, size_t n, uint8_t *bwt_out, uint32_t *ptr,
                       uint8_t *has_byte)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || !ptr || !has_byte) return BZH_E_ARG;
    if (n == 0) { // lib/bwt.rs:535-541
        memset(has_byte, 0, 256);
        *ptr = UINT32_MAX;
        return BZH_OK;
    }
    if (n > ctx->M) return BZH_E_ARG;
    uint64_t off = 0;
    uint32_t len = (uint32_t)n;
    return bzh_bwt_batch(ctx, in, &off, &len, 1, bwt_out, ptr, has_byte);
    });
}

// ---- verification tooling: inverse BWT -----------------------------------------------
extern "C" int bzh_unbwt_batch(bzh_ctx *ctx, const uint8_t *bwt, const uint64_t *offs, const uint32_t *lens,
                               const uint32_t *ptr, size_t nblk, uint8_t *out)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || !bwt || !offs || !lens || !ptr || !out) return BZH_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    BZH_TRY(ensure_arena(ctx, (uint32_t)std::min<size_t>(nblk, ctx->max_batch)));
    Batch &bt = ctx->bt;
    for (size_t k0 = 0; k0 < nblk; k0 += ctx->max_batch) {
        const uint32_t B = (uint32_t)std::min<size_t>(ctx->max_batch, nblk - k0);
        uint32_t nmax = 0;
        for (uint32_t b = 0; b < B; b++) {
            const uint32_t n = lens[k0 + b];
            if (n == 0 || n > ctx->M || ptr[k0 + b] >= n) {
                bzh_set_error(ctx, "block %zu: length %u / pointer %u out of range", k0 + b, n, ptr[k0 + b]);
                return BZH_E_ARG;
            }
            nmax = std::max(nmax, n);
            HIP_TRY(ctx, hipMemcpyAsync(bt.bwt + (size_t)b * bt.S, bwt + offs[k0 + b], n, hipMemcpyHostToDevice, ctx->stream));
        }
        HIP_TRY(ctx, hipMemcpyAsync(bt.n, lens + k0, B * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(bt.ptr, ptr + k0, B * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        BZH_TRY(unbwt_run(ctx, B, nmax));
        for (uint32_t b = 0; b < B; b++)
            HIP_TRY(ctx, hipMemcpyAsync(out + offs[k0 + b], bt.unbwt_out + (size_t)b * bt.S, lens[k0 + b], hipMemcpyDeviceToHost,
                                        ctx->stream));
        HIP_TRY(ctx, bzh_stream_wait(ctx->stream));
    }
    return BZH_OK;
    });
}

// Forward + inverse transform of plan blocks [b0, b1) entirely on the device: RLE1 bytes -> BWT -> inverse BWT,
// compared with the RLE1 bytes.  *mismatches = differing bytes (0 for a correct transform).
extern "C" int bzh_bwt_roundtrip_device(bzh_ctx *ctx, size_t b0, size_t b1, uint64_t *mismatches)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || !mismatches || b0 > b1) return BZH_E_ARG;
    if (b1 > ctx->plan_blocks.size()) return BZH_E_STATE;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    ctx->evnext = 0; // (the pool is reused from the start by every entry point that takes events)
    ctx->sort_spans.clear(); // (spans recorded against the old use of those events must not survive the rewind)
    kstats_reset(ctx);
    BZH_TRY(ensure_arena(ctx, (uint32_t)std::min<size_t>(b1 - b0, ctx->max_batch)));
    unsigned long long *d_acc = ctx->bt.stat_A; // (the forward sort has read it back by the time it is reused)
    unsigned long long total = 0;
    for (size_t k0 = b0; k0 < b1; k0 += ctx->max_batch) {
        const uint32_t B = (uint32_t)std::min<size_t>(ctx->max_batch, b1 - k0);
        const BzeSums s = bze_job_sums(ctx->plan_blocks.data(), k0, B);
        BZH_TRY(rle1_emit(ctx, k0, B));
        BZH_TRY(bwt_run(ctx, B, s.nmax, s.ntotal));
        BZH_TRY(unbwt_run(ctx, B, s.nmax));
        HIP_TRY(ctx, hipMemsetAsync(d_acc, 0, sizeof(unsigned long long), st));
        BZH_TRY(unbwt_compare(ctx, B, s.nmax, d_acc));
        unsigned long long part = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&part, d_acc, sizeof part, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, bzh_stream_wait(st));
        total += part;
    }
    *mismatches = total;
    return BZH_OK;
    });
}

// ---- stage seam: MTF + RLE2 ---------------------------------------------------------------------------
// All nblk columns run in ONE mtf_run, so nblk alone decides the tile size (mtf_tile_bytes): verification tooling that
// brings chosen columns to the tiles of batches of 64 blocks and more, which whole streams reach only with the columns
// their BWT happens to give.  Block k's symbols go to syms[offs[k] + k ..), lens[k] + 1 entries of room.
extern "C" int bzh_mtf_batch(bzh_ctx *ctx, const uint8_t *bwt, const uint64_t *offs, const uint32_t *lens, size_t nblk,
                             const uint8_t *has_byte, uint16_t *syms, uint32_t *m, uint32_t *freqs, uint32_t *num_syms)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx) return BZH_E_ARG;
    if (!bwt || !offs || !lens || !has_byte || !syms || !m || !freqs || !num_syms) {
        bzh_set_error(ctx, "bzh_mtf_batch: null pointer");
        return BZH_E_ARG;
    }
    if (nblk == 0 || nblk > ctx->max_batch) {
        bzh_set_error(ctx, "bzh_mtf_batch: %zu blocks outside 1..%u", nblk, ctx->max_batch);
        return BZH_E_ARG;
    }
    const uint32_t B = (uint32_t)nblk;
    uint32_t nmax = 0;
    uint64_t ntotal = 0;
    for (uint32_t b = 0; b < B; b++) {
        if (lens[b] == 0 || lens[b] > ctx->M) {
            bzh_set_error(ctx, "block %u length %u outside 1..%u", b, lens[b], ctx->M);
            return BZH_E_ARG;
        }
        nmax = std::max(nmax, lens[b]);
        ntotal += lens[b];
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    stats_begin(ctx);
    BZH_TRY(ensure_arena(ctx, B));
    Batch &bt = ctx->bt;
    hipStream_t st = ctx->stream;
    for (uint32_t b = 0; b < B; b++)
        HIP_TRY(ctx, hipMemcpyAsync(bt.bwt + (size_t)b * bt.S, bwt + offs[b], lens[b], hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(bt.n, lens, B * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(bt.hasbyte, has_byte, (size_t)B * 256, hipMemcpyHostToDevice, st));
    BZH_TRY(mtf_run(ctx, B, nmax, ntotal));
    HIP_TRY(ctx, hipMemcpyAsync(m, bt.m, B * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(num_syms, bt.nsyms, B * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(freqs, bt.freqs, (size_t)B * 258 * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, bzh_stream_wait(st));
    for (uint32_t b = 0; b < B; b++) {
        if (m[b] == 0 || m[b] > lens[b] + 1) {
            bzh_set_error(ctx, "mtf produced m=%u for n=%u (block %u)", m[b], lens[b], b);
            return BZH_E_HIP;
        }
    }
    for (uint32_t b = 0; b < B; b++)
        HIP_TRY(ctx, hipMemcpyAsync(syms + offs[b] + b, bt.syms + (size_t)b * (bt.S + 64), (size_t)m[b] * sizeof(uint16_t),
                                    hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, bzh_stream_wait(st));
    return BZH_OK;
    });
}

extern "C" int bzh_mtf(bzh_ctx *ctx, const uint8_t *bwt, size_t n, const uint8_t *has_byte, uint16_t *syms,
                       size_t *m, uint32_t *freqs, uint32_t *num_syms)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || !bwt || !has_byte || !syms || !m || !freqs || !num_syms || n == 0 || n > ctx->M) return BZH_E_ARG;
    const uint64_t off = 0;
    const uint32_t len = (uint32_t)n;
    uint32_t m32 = 0;
    const int rc = bzh_mtf_batch(ctx, bwt, &off, &len, 1, has_byte, syms, &m32, freqs, num_syms);
    if (rc == BZH_OK) *m = m32;
    return rc;
    });
}

// ---- stage seam: Huffman ----------------------------------------------------------------------------------
// The device path always writes a whole block (header + symbol map + payload).  For the seam the
// block is built with a fixed dummy header (crc 0, ptr 0, only byte 0 present: 105 + 32 bits) and
// the host strips those 137 bits, leaving exactly what huffman::encode writes (lib/huffman.rs:464-572).
extern "C" int bzh_huffman(bzh_ctx *ctx, const uint16_t *syms, size_t m, uint32_t num_syms, const uint32_t *freqs,
                           uint8_t *bits_out, size_t cap, uint64_t *nbits, uint8_t *code_lengths,
                           uint32_t *num_tables)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || !syms || !freqs || !bits_out || !nbits || m == 0 || m > (size_t)ctx->M + 1 || num_syms < 3 ||
        num_syms > 258)
        return BZH_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    stats_begin(ctx);
    struct ModeGuard { // the seam is the reference's huffman::encode whatever mode the context is in
        bzh_ctx *c;
        int keep;
        ~ModeGuard() { c->mode = keep; }
    } guard{ctx, ctx->mode};
    ctx->mode = BZH_MODE_REFERENCE;
    BZH_TRY(ensure_arena(ctx, 1));
    Batch &bt = ctx->bt;
    hipStream_t st = ctx->stream;
    const uint32_t m32 = (uint32_t)m;
    uint8_t hb[256] = {1};
    BlockDesc d{};
    uint32_t zero = 0;
    HIP_TRY(ctx, hipMemcpyAsync(bt.syms, syms, m * sizeof(uint16_t), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(bt.m, &m32, 4, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(bt.nsyms, &num_syms, 4, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(bt.freqs, freqs, 258 * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(bt.hasbyte, hb, 256, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(bt.desc, &d, sizeof d, hipMemcpyHostToDevice, st));
    bt.pdesc = bt.desc;
    HIP_TRY(ctx, hipMemcpyAsync(bt.ptr, &zero, 4, hipMemcpyHostToDevice, st));
    BZH_TRY(huff_prepare(ctx, 1, m32));
    uint64_t total = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&total, bt.bitoff + 1, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, bzh_stream_wait(st));
    const size_t bytes = (size_t)((total + 31) / 32 * 4);
    BZH_TRY(ensure_stage(ctx, ctx->d_stage_out, bytes));
    HIP_TRY(ctx, hipMemsetAsync(ctx->d_stage_out, 0, bytes, st));
    BZH_TRY(huff_pack(ctx, 1, m32, ctx->d_stage_out, 0));
    std::vector<uint8_t> tmp(bytes + 8, 0);
    HIP_TRY(ctx, hipMemcpyAsync(tmp.data(), ctx->d_stage_out, bytes, hipMemcpyDeviceToHost, st));
    uint32_t nt = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&nt, bt.ntab, 4, hipMemcpyDeviceToHost, st));
    if (code_lengths) HIP_TRY(ctx, hipMemcpyAsync(code_lengths, bt.lens, 3 * 258, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, bzh_stream_wait(st));
    if (num_tables) *num_tables = nt;
    const uint64_t skip = 105 + 32;
    const uint64_t pay = total - skip;
    *nbits = pay;
    const size_t need = (size_t)((pay + 7) / 8);
    if (need > cap) return BZH_E_CAP;
    for (size_t k = 0; k < need; k++) { // shift left by 137 bits = 17 bytes + 1 bit
        const size_t src = k + skip / 8;
        const unsigned sh = skip % 8;
        bits_out[k] = (uint8_t)((tmp[src] << sh) | (tmp[src + 1] >> (8 - sh)));
    }
    if (pay % 8) bits_out[need - 1] &= (uint8_t)(0xFF << (8 - pay % 8));
    return BZH_OK;
    });
}

// ================================================================================================
// Whole path
// ================================================================================================
__device__ __forceinline__ void or_word_be(uint32_t *out, uint64_t word_idx, uint32_t v)
{
    if (v) atomicOr(out + word_idx, __builtin_bswap32(v));
}

// Copies nbits bits of src (MSB-first, from bit 0) to bit position dst_bit of dst (zeroed before).
// One thread per DESTINATION word: interior words are plain stores assembled from two source words
// (funnel shift); only the first and last word, shared with the neighbouring segments, are ORed.
__global__ void __launch_bounds__(256) concat_bits(uint32_t *dst, uint64_t dst_bit, const uint32_t *src, uint64_t nbits)
{
    const uint32_t sh = (uint32_t)(dst_bit & 31u);
    const uint64_t w0 = dst_bit >> 5;
    const uint64_t nsw = (nbits + 31) >> 5;            // source words
    const uint64_t ndw = (sh + nbits + 31) >> 5;       // destination words touched
    const uint32_t tailbits = (uint32_t)(nbits & 31u);
    for (uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x; k < ndw; k += (uint64_t)gridDim.x * 256) {
        // destination word k holds source bits [32k - sh, 32k - sh + 32)
        uint32_t hi = 0, lo = 0; // source words k-1 and k (big-endian values)
        if (k >= 1 && k - 1 < nsw) {
            hi = __builtin_bswap32(src[k - 1]);
            if (k - 1 == nsw - 1 && tailbits) hi &= 0xFFFFFFFFu << (32 - tailbits);
        }
        if (k < nsw) {
            lo = __builtin_bswap32(src[k]);
            if (k == nsw - 1 && tailbits) lo &= 0xFFFFFFFFu << (32 - tailbits);
        }
        const uint32_t v = sh ? ((hi << (32 - sh)) | (lo >> sh)) : lo;
        if (k == 0 || k == ndw - 1)
            or_word_be(dst, w0 + k, v);
        else
            dst[w0 + k] = __builtin_bswap32(v);
    }
}

// Stream header "BZh"+level at bit 0 and footer + stream CRC at bit 32+body_bits (lib/lib.rs:18-22, :66-70).
__global__ void stream_frame(uint32_t *out, int level, uint64_t body_bits, uint32_t stream_crc)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    or_word_be(out, 0, 0x425A6800u | (uint32_t)('0' + level));
    const uint32_t words[3] = {0x17724538u, 0x50900000u | (stream_crc >> 16), stream_crc << 16}; // 80 bits
    const uint64_t pos = 32 + body_bits;
    const uint32_t sh = (uint32_t)(pos & 31u);
    const uint64_t w0 = pos >> 5;
    for (int k = 0; k < 3; k++) {
        or_word_be(out, w0 + k, words[k] >> sh);
        if (sh) or_word_be(out, w0 + k + 1, words[k] << (32 - sh));
    }
}

static uint32_t fold_stream_crc(const uint32_t *crcs, size_t nb) // lib/lib.rs:107-108
{
    uint32_t s = 0;
    for (size_t k = 0; k < nb; k++) s = crcs[k] ^ ((s << 1) | (s >> 31));
    return s;
}

static float span_ms(hipEvent_t a, hipEvent_t b)
{
    float t = 0;
    return hipEventElapsedTime(&t, a, b) == hipSuccess ? t : 0.f;
}

// ---- lanes: two half-batch workers so that one half's latency-bound phases (tail rounds of the
// suffix sort, the Huffman heap, per-round read-backs) overlap the other half's bandwidth-bound kernels
static int ensure_lanes(bzh_ctx *ctx)
{
    if (!ctx->lanes.empty()) return BZH_OK;
    const uint32_t lane_mb = std::max<uint32_t>(1, ctx->max_batch / 2);
    Batch probe{};
    const size_t half = layout_batch(probe, nullptr, lane_mb, ctx->M);
    BZH_TRY(ensure_arena(ctx, ctx->max_batch, 2 * half)); // the lanes share the full-size arena, half each
    for (int k = 0; k < 2; k++) {
        bzh_ctx *l = new (std::nothrow) bzh_ctx();
        if (!l) return BZH_E_NOMEM;
        l->parent = ctx;
        l->device = ctx->device;
        l->level = ctx->level;
        l->M = ctx->M;
        l->max_batch = lane_mb;
        l->mode = ctx->mode;
        layout_batch(l->bt, ctx->arena.p + (size_t)k * half, lane_mb, ctx->M);
        l->S = l->bt.S;
        if (hipStreamCreateWithFlags(&l->stream, hipStreamNonBlocking) != hipSuccess || pinned_alloc(l) != BZH_OK) {
            delete l;
            return BZH_E_NOMEM;
        }
        ctx->lanes.push_back(l);
    }
    return BZH_OK;
}

struct RangeJob {
    size_t k0 = 0;
    uint32_t B = 0, nmax = 0, mmax = 0;
    uint64_t ntotal = 0, T = 0;
    int status = BZH_OK;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
};

// Plan blocks [b0, b1) as jobs of `per` blocks (encode_plan.h), counted into the call's statistics.
static void build_jobs(bzh_ctx *ctx, size_t b0, size_t b1, size_t per, std::vector<RangeJob> &jobs)
{
    std::vector<BzeSpan> spans;
    bze_split(b0, b1, per, spans);
    for (const BzeSpan &sp : spans) {
        const BzeSums s = bze_job_sums(ctx->plan_blocks.data(), sp.k0, sp.B);
        ctx->stats.rle_bytes += s.ntotal;
        ctx->stats.raw_bytes += s.raw;
        ctx->stats.blocks += sp.B;
        jobs.push_back({sp.k0, sp.B, s.nmax, s.mmax, s.ntotal});
    }
}

// The jobs' events -> the stage times of the call (profiling; the streams have been waited for).
static void jobs_ms(bzh_ctx *ctx, const std::vector<RangeJob> &jobs)
{
    for (const RangeJob &job : jobs) {
        ctx->stats.ms_rle1 += span_ms(job.ev[0], job.ev[1]);
        ctx->stats.ms_bwt += span_ms(job.ev[1], job.ev[2]);
        ctx->stats.ms_mtf += span_ms(job.ev[2], job.ev[3]);
        ctx->stats.ms_huff += span_ms(job.ev[3], job.ev[4]);
        ctx->stats.ms_pack += span_ms(job.ev[4], job.ev[5]);
    }
}

// Everything of a batch up to its bit total, on the lane's stream and arena.
static int prepare_batch(bzh_ctx *lane, RangeJob &j, bool wait_total = true)
{
    hipStream_t st = lane->stream;
    lane->k_cur_ntotal = j.ntotal;
    j.ev[0] = call_mark(lane);
    BZH_TRY(rle1_emit(lane, j.k0, j.B));
    j.ev[1] = call_mark(lane);
    BZH_TRY(bwt_run(lane, j.B, j.nmax, j.ntotal));
    j.ev[2] = call_mark(lane);
    BZH_TRY(mtf_run(lane, j.B, j.nmax, j.ntotal));
    j.ev[3] = call_mark(lane);
    {   // the block headers carry the block CRCs: a whole-path plan left them to the owner's second stream (rle1_plan_split)
        bzh_ctx *pc = lane->parent ? lane->parent : lane;
        if (pc->crc_pending) HIP_TRY(lane, hipStreamWaitEvent(st, pc->plan_ev[1], 0));
    }
    BZH_TRY(huff_prepare(lane, j.B, j.mmax));
    j.ev[4] = call_mark(lane);
    if (!wait_total) return BZH_OK; // (a call of one batch: the device carries on by itself, encode_range reads the total at the end)
    HIP_TRY(lane, hipMemcpyAsync(&j.T, lane->bt.bitoff + j.B, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(lane, bzh_stream_wait(st));
    return BZH_OK;
}

// Two lanes: lane k prepares jobs k, k + 2, ... on a thread of its own while this thread packs them in order; a lane may reuse
// its arena only after its job was packed.  -> the first failure (`keep`: the statistics to go back to where no thread could be
// started)
template <typename Pack>
static int run_lanes(bzh_ctx *ctx, const std::vector<bzh_ctx *> &lanes, std::vector<RangeJob> &jobs, const bzh_stats &keep, Pack &&pack)
{
    struct Turn {
        std::promise<void> ready, packed;
    };
    const size_t NL = lanes.size();
    std::vector<Turn> turns(jobs.size());
    std::atomic<bool> abort{false}; // set when not every lane thread could be started: the ones that did start do nothing
    auto worker = [&](int k) {
        hipSetDevice(ctx->device);
        bool dead = false;
        for (size_t j = k; j < jobs.size(); j += NL) {
            jobs[j].status = (dead || abort.load()) ? BZH_E_STATE : prepare_batch(lanes[k], jobs[j]);
            if (jobs[j].status != BZH_OK) dead = true;
            turns[j].ready.set_value();
            turns[j].packed.get_future().wait();
        }
    };
    std::vector<std::thread> threads;
    try {
        threads.reserve(NL);
        for (size_t k = 0; k < NL; k++) threads.emplace_back(worker, (int)k);
    } catch (...) { // no thread to be had: release the workers that did start (they skip their jobs), then report
        abort.store(true);
        for (Turn &t : turns) t.packed.set_value();
        for (auto &t : threads) t.join();
        for (bzh_ctx *l : lanes) hipStreamSynchronize(l->stream); // (a job may have been in flight already)
        ctx->stats = keep;
        bzh_set_error(ctx, "could not start the lane threads");
        return BZH_E_NOMEM;
    }
    int status = BZH_OK;
    for (size_t j = 0; j < jobs.size(); j++) {
        bzh_ctx *lane = lanes[j % NL];
        turns[j].ready.get_future().wait();
        if (status == BZH_OK && jobs[j].status != BZH_OK) {
            status = jobs[j].status;
            bzh_set_error(ctx, "%s", lane->err);
        }
        if (status == BZH_OK) status = pack(lane, jobs[j]);
        turns[j].packed.set_value();
    }
    for (auto &t : threads) t.join();
    return status;
}

// Encodes plan blocks [b0, b1) into d_out starting at bit `bit_base`; words of d_out from
// bit_base/32 on are zeroed here as needed (words before that are the caller's).
// (`framed`: in/out -- the caller wants the whole stream's header and footer around these blocks; set back to false unless
// this call wrote them on the device: one batch, one lane, all blocks of the plan from bit 32 on)
// (`ix`: the caller wants the index of what is written -- bzh_encode_index*; every batch is handed to sync_emit_batch behind its
// pack, while its arena still holds it; one lane whatever bzh_set_lanes says)
static int encode_range(bzh_ctx *ctx, size_t b0, size_t b1, uint8_t *d_out, size_t cap, uint64_t bit_base,
                        uint64_t *nbits, const uint32_t *seed_word = nullptr, bool *framed = nullptr, EncIndex *ix = nullptr)
{
    const bool want_frame = framed && *framed;
    if (framed) *framed = false;
    if (((uintptr_t)d_out & 3u) != 0) {
        bzh_set_error(ctx, "output buffer must be 4-byte aligned");
        return BZH_E_ARG;
    }
    // default: one lane = this context (whole arena, caller's stream, no extra threads)
    std::vector<bzh_ctx *> lanes{ctx};
    if (ctx->nlanes == 2 && !ix) {
        BZH_TRY(ensure_lanes(ctx));
        lanes = ctx->lanes;
    }
    const size_t NL = lanes.size();
    if (NL > 1) HIP_TRY(ctx, bzh_stream_wait(ctx->stream)); // the plan and whatever produced the input: the lanes' streams start behind it (one lane = this stream: in order anyway)
    const bzh_stats keep = ctx->stats; // what the counters were before this call touched them
    const size_t per = bze_per(b1 - b0, lanes[0]->max_batch, NL);
    if (NL == 1) BZH_TRY(ensure_arena(ctx, (uint32_t)per));
    std::vector<RangeJob> jobs;
    build_jobs(ctx, b0, b1, per, jobs);
    for (bzh_ctx *l : lanes) {
        l->profiling = ctx->profiling;
        if (l != ctx) {
            stats_begin(l);
            l->err[0] = 0;
        } else {
            ctx->sort_spans.clear();
            ctx->stats.bwt_active_sum = 0;
            ctx->stats.bwt_rounds = 0;
            ctx->stats.bwt_sort_launches = 0;
            ctx->stats.bwt_sort_elems = 0;
        }
    }

    const uint64_t cap_words = cap / 4;
    uint64_t zeroed_upto = bit_base / 32; // first word not yet known to be zero
    uint64_t cur = 0;
    // A call of ONE batch (the usual case: up to max_batch blocks) needs the host for nothing between the Huffman tables and
    // the packed bits: the output words are zeroed, the capacity checked and the pack kernels gated on the device
    // (huff_pack_gate), and the bit total is read once, at the end -- instead of a copy, a wait, a memset and a launch in the
    // middle of the step (35-40 us of idle device).  With several batches the host has every batch's total before its pack
    // (prepare_batch waited for it: the next batch's position depends on it), so it zeroes and checks the capacity itself.
    const bool gated = NL == 1 && jobs.size() == 1;
    // The pack step of one job, behind its prepare_batch: the job's bits at bit_base + cur, the lane's arena free again.
    auto pack = [&](bzh_ctx *lane, RangeJob &job) -> int {
        hipStream_t st = lane->stream;
        uint64_t *rec = lane->h_pinned.as<uint64_t>(); // (the first 64 words of the pinned block are free)
        const uint64_t at = bit_base + cur;
        bool over = false;
        hipError_t he = hipSuccess;
        int rc = BZH_OK;
        if (gated) {
            const bool frame = want_frame && bit_base == 32 && b0 == 0 && !seed_word; // (block CRCs of the batch = of the stream)
            rc = huff_pack_gate(lane, job.B, d_out, at, cap_words, seed_word ? *seed_word : 0u, seed_word != nullptr, rec, frame ? 80u : 0u);
            if (rc == BZH_OK) rc = huff_pack(lane, job.B, job.mmax, d_out, at, true);
            if (rc == BZH_OK && frame && (rc = huff_frame_stream(lane, job.B, d_out)) == BZH_OK) *framed = true;
        } else {
            const BzeZero z = bze_zero_batch(bit_base, cur, job.T, zeroed_upto, cap_words);
            over = z.over;
            if (!over && z.to > z.from) {
                he = hipMemsetAsync(d_out + z.from * 4, 0, (size_t)(z.to - z.from) * 4, st);
                if (he == hipSuccess && seed_word && z.from == bit_base / 32) // bits owed to the first word
                    he = hipMemcpyAsync(d_out + z.from * 4, seed_word, 4, hipMemcpyHostToDevice, st);
                zeroed_upto = z.to;
            }
            if (!over && he == hipSuccess) rc = huff_pack(lane, job.B, job.mmax, d_out, at);
        }
        if (rc != BZH_OK) {
            (void)bzh_stream_wait(st); // (nothing of this call may still run when the error is reported)
            return rc;
        }
        std::vector<uint32_t> hm;
        if (!over) {
            if (lane->profiling && he == hipSuccess) {
                job.ev[5] = call_mark(lane);
                hm.resize(job.B);
                he = hipMemcpyAsync(hm.data(), lane->bt.m, job.B * 4, hipMemcpyDeviceToHost, st);
            }
            if (he == hipSuccess) he = bzh_stream_wait(st); // the lane's arena is free again
            if (he != hipSuccess) {
                bzh_set_error(ctx, "pack: %s", hipGetErrorString(he));
                return BZH_E_HIP;
            }
            if (gated) { // what the gate found: the batch's bits, and whether they fit
                __atomic_thread_fence(__ATOMIC_ACQUIRE);
                job.T = reinterpret_cast<volatile uint64_t *>(rec)[0];
                over = reinterpret_cast<volatile uint64_t *>(rec)[1] == 0;
            }
        }
        if (over) {
            bzh_set_error(ctx, "output needs more than %zu bytes", cap);
            return BZH_E_CAP;
        }
        for (uint32_t m : hm) ctx->stats.mtf_syms += m;
        if (ix) BZH_TRY(sync_emit_batch(lane, job.B, job.k0, at, *ix));
        cur += job.T;
        return BZH_OK;
    };
    if (NL == 1) {
        for (RangeJob &job : jobs) {
            BZH_TRY(prepare_batch(ctx, job, !gated));
            BZH_TRY(pack(ctx, job));
        }
    } else {
        BZH_TRY(run_lanes(ctx, lanes, jobs, keep, pack));
    }
    if (ctx->profiling) {
        jobs_ms(ctx, jobs);
        for (bzh_ctx *l : lanes) {
            stats_collect_sort(l);
            if (l == ctx) continue;
            ctx->stats.ms_bwt_sort += l->stats.ms_bwt_sort;
            ctx->stats.bwt_sort_launches += l->stats.bwt_sort_launches;
            ctx->stats.bwt_sort_elems += l->stats.bwt_sort_elems;
            for (int k = 0; k < K_COUNT; k++) {
                ctx->k_ms[k] += l->k_ms[k];
                ctx->k_bytes[k] += l->k_bytes[k];
                ctx->k_launch[k] += l->k_launch[k];
            }
        }
    }
    for (bzh_ctx *l : lanes) {
        if (l == ctx) continue;
        ctx->stats.bwt_active_sum += l->stats.bwt_active_sum;
        ctx->stats.bwt_rounds = std::max(ctx->stats.bwt_rounds, l->stats.bwt_rounds);
    }
    ctx->stats.out_bits += cur;
    *nbits = cur;
    return BZH_OK;
}

static int check_in_ptr(bzh_ctx *ctx, const void *d_in)
{
    if (((uintptr_t)d_in & 15u) != 0) {
        bzh_set_error(ctx, "device input must be 16-byte aligned");
        return BZH_E_ARG;
    }
    return BZH_OK;
}

static int plan_device(bzh_ctx *ctx, const void *d_in, size_t n, size_t *nblocks, bool with_crc)
{
    if (ctx) stream_join(ctx);
    if (!ctx || (!d_in && n) || !nblocks) return BZH_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    BZH_TRY(check_in_ptr(ctx, d_in));
    if (ctx->profiling) ctx->evnext = 0;
    hipEvent_t e0 = call_mark(ctx);
    BZH_TRY(rle1_plan(ctx, (const uint8_t *)d_in, n, with_crc));
    if (ctx->profiling) {
        hipEvent_t e1 = call_mark(ctx);
        HIP_TRY(ctx, bzh_stream_wait(ctx->stream));
        memset(&ctx->stats, 0, sizeof ctx->stats);
        ctx->stats.ms_plan = span_ms(e0, e1);
    }
    *nblocks = ctx->plan_blocks.size();
    return BZH_OK;
}

extern "C" int bzh_plan_device(bzh_ctx *ctx, const void *d_in, size_t n, size_t *nblocks)
{
    return bzh_guard(ctx, [&]() -> int {
    return plan_device(ctx, d_in, n, nblocks, true);
    });
}

extern "C" int bzh_plan_device_nocrc(bzh_ctx *ctx, const void *d_in, size_t n, size_t *nblocks)
{
    return bzh_guard(ctx, [&]() -> int {
    return plan_device(ctx, d_in, n, nblocks, false);
    });
}

extern "C" int bzh_plan_tables_device(bzh_ctx *ctx, const void *d_in, size_t n)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || (!d_in && n)) return BZH_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    BZH_TRY(check_in_ptr(ctx, d_in));
    if (ctx->profiling) {
        ctx->evnext = 0;
        kstats_reset(ctx);
    }
    return rle1_plan_tables(ctx, (const uint8_t *)d_in, n);
    });
}

extern "C" int bzh_plan_split_device(bzh_ctx *ctx, size_t start, size_t stop, int with_crc, size_t *nblocks)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || !nblocks) return BZH_E_ARG;
    if (start > ctx->plan_n) return BZH_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    BZH_TRY(rle1_plan_split(ctx, start, with_crc != 0, stop));
    *nblocks = ctx->plan_blocks.size();
    return BZH_OK;
    });
}

extern "C" int bzh_plan_crc_range(bzh_ctx *ctx, size_t b0, size_t b1)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || b0 > b1) return BZH_E_ARG;
    if (b1 > ctx->plan_blocks.size()) return BZH_E_STATE;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return rle1_plan_crc(ctx, b0, b1);
    });
}

extern "C" int bzh_plan_open(const bzh_ctx *ctx, uint8_t *out, size_t max_blocks)
{
    return bzh_guard(const_cast<bzh_ctx *>(ctx), [&]() -> int {
    if (!ctx || !out) return BZH_E_ARG;
    if (max_blocks < ctx->plan_open.size()) return BZH_E_CAP;
    for (size_t k = 0; k < ctx->plan_open.size(); k++) out[k] = ctx->plan_open[k];
    return BZH_OK;
    });
}

extern "C" int bzh_plan_blocks(const bzh_ctx *ctx, bzh_block *out, size_t max_blocks)
{
    return bzh_guard(const_cast<bzh_ctx *>(ctx), [&]() -> int {
    if (!ctx || !out) return BZH_E_ARG;
    if (max_blocks < ctx->plan_blocks.size()) return BZH_E_CAP;
    const bool many = ctx->plan_input.size() == ctx->plan_blocks.size(); // (a plan of many inputs: offsets in its guarded buffer)
    for (size_t k = 0; k < ctx->plan_blocks.size(); k++) {
        out[k] = ctx->plan_blocks[k];
        if (many) out[k].in_off -= ctx->plan_input[k];
    }
    return BZH_OK;
    });
}

extern "C" int bzh_encode_range_device(bzh_ctx *ctx, size_t b0, size_t b1, void *d_out, size_t cap,
                                       uint64_t *nbits)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || !d_out || !nbits || b0 > b1) return BZH_E_ARG;
    if (b1 > ctx->plan_blocks.size()) return BZH_E_STATE;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    BZH_TRY(stats_begin(ctx, true));
    *nbits = 0;
    if (b0 == b1) return BZH_OK;
    BZH_TRY(rle1_plan_crc(ctx, b0, b1)); // no-op unless the plan left the CRCs to the encoder
    return encode_range(ctx, b0, b1, (uint8_t *)d_out, cap, 0, nbits);
    });
}

extern "C" int bzh_assemble_device(bzh_ctx *ctx, const void *const *d_segs, const uint64_t *seg_bits, size_t nseg,
                                   const uint32_t *block_crcs, size_t nblocks, void *d_out, size_t cap,
                                   size_t *out_len)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || !d_out || !out_len || (nseg && (!d_segs || !seg_bits)) || (nblocks && !block_crcs)) return BZH_E_ARG;
    if (((uintptr_t)d_out & 3u) != 0) return BZH_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    uint64_t body = 0;
    for (size_t k = 0; k < nseg; k++) body += seg_bits[k];
    const uint64_t total_bits = 32 + body + 80;
    const size_t bytes = (size_t)((total_bits + 7) / 8);
    const size_t words = (size_t)((total_bits + 31) / 32) + 1;
    *out_len = bytes;
    if (words * 4 > cap) return BZH_E_CAP;
    HIP_TRY(ctx, hipMemsetAsync(d_out, 0, words * 4, st));
    uint64_t pos = 32;
    for (size_t k = 0; k < nseg; k++) {
        if (seg_bits[k] == 0) continue;
        if (((uintptr_t)d_segs[k] & 3u) != 0) return BZH_E_ARG;
        const uint64_t nw = (seg_bits[k] + 31) / 32 + 1;
        uint32_t grid = (uint32_t)std::min<uint64_t>((nw + 255) / 256, 8192);
        concat_bits<<<dim3(grid), 256, 0, st>>>((uint32_t *)d_out, pos, (const uint32_t *)d_segs[k], seg_bits[k]);
        pos += seg_bits[k];
    }
    stream_frame<<<1, 64, 0, st>>>((uint32_t *)d_out, ctx->level, body, fold_stream_crc(block_crcs, nblocks));
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, bzh_stream_wait(st));
    return BZH_OK;
    });
}

// bzh_encode_device; with `ix` also the index of the stream (bzh_encode_index_device)
static int encode_device_impl(bzh_ctx *ctx, const void *d_in, size_t n, void *d_out, size_t cap, size_t *out_len, size_t *consumed,
                              EncIndex *ix)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || (!d_in && n) || !d_out || !out_len) return BZH_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (((uintptr_t)d_out & 3u) != 0 || cap < 16) return BZH_E_ARG;
    stats_begin(ctx);
    hipEvent_t t0 = call_mark(ctx);
    BZH_TRY(check_in_ptr(ctx, d_in));
    BZH_TRY(rle1_plan(ctx, (const uint8_t *)d_in, n, true, true)); // (the block CRCs beside the main stream: joined below)
    hipEvent_t t1 = call_mark(ctx);
    // words 0 and 1 hold the stream header and the first body bits
    HIP_TRY(ctx, hipMemsetAsync(d_out, 0, 4, st));
    uint64_t body = 0;
    const size_t nb = ctx->plan_blocks.size();
    bool framed = true; // (a stream of one batch gets its header and footer on the device, behind the pack: no host round trip)
    if (nb) {
        if (ix) BZH_TRY(rle1_plan_crc_join(ctx)); // (the entries carry the block CRCs)
        BZH_TRY(encode_range(ctx, 0, nb, (uint8_t *)d_out, cap, 32, &body, nullptr, &framed, ix));
    } else {
        framed = false;
        HIP_TRY(ctx, hipMemsetAsync(d_out, 0, 16, st));
    }
    const uint64_t total_bits = 32 + body + 80;
    const size_t bytes = (size_t)((total_bits + 7) / 8);
    *out_len = bytes;
    if (framed) { // (everything is written and waited for; the CRCs are collected for bzh_plan_blocks' sake)
        BZH_TRY(rle1_plan_crc_join(ctx));
    } else {
        // the footer may reach one word past what encode_range zeroed
        const BzeZero z = bze_zero_footer(32 + body, nb != 0, cap / 4);
        if (z.over) return BZH_E_CAP;
        if (z.to > z.from) HIP_TRY(ctx, hipMemsetAsync((uint8_t *)d_out + z.from * 4, 0, (size_t)(z.to - z.from) * 4, st));
        BZH_TRY(rle1_plan_crc_join(ctx));
        std::vector<uint32_t> crcs(nb);
        for (size_t k = 0; k < nb; k++) crcs[k] = ctx->plan_blocks[k].crc;
        stream_frame<<<1, 64, 0, st>>>((uint32_t *)d_out, ctx->level, body, fold_stream_crc(crcs.data(), nb));
        HIP_TRY(ctx, hipGetLastError());
    }
    hipEvent_t t2 = call_mark(ctx);
    if (!framed || ctx->profiling) HIP_TRY(ctx, bzh_stream_wait(st));
    if (ctx->profiling) {
        ctx->stats.ms_plan = span_ms(t0, t1);
        ctx->stats.ms_total = span_ms(t0, t2);
    }
    if (consumed) *consumed = n;
    return BZH_OK;
    });
}

extern "C" int bzh_encode_device(bzh_ctx *ctx, const void *d_in, size_t n, void *d_out, size_t cap, size_t *out_len,
                                 size_t *consumed)
{
    return encode_device_impl(ctx, d_in, n, d_out, cap, out_len, consumed, nullptr);
}

// bzh_encode; with `ix` also the index of the stream (bzh_encode_index): host buffers, through the staging buffers
static int encode_host(bzh_ctx *ctx, const uint8_t *in, size_t n, uint8_t *out, size_t cap, size_t *out_len, size_t *consumed,
                       EncIndex *ix)
{
    if (ctx) stream_join(ctx);
    if (!ctx || (!in && n) || !out || !out_len) return BZH_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    BZH_TRY(ensure_stage(ctx, ctx->d_stage_in, n + 16));
    const size_t dcap = n + n / 4 + (n / ((size_t)ctx->M * 4 / 5) + 2) * 4096 + 65536;
    BZH_TRY(ensure_stage(ctx, ctx->d_stage_out, dcap));
    if (n) HIP_TRY(ctx, hipMemcpyAsync(ctx->d_stage_in, in, n, hipMemcpyHostToDevice, st));
    size_t len = 0;
    BZH_TRY(encode_device_impl(ctx, ctx->d_stage_in, n, ctx->d_stage_out, ctx->d_stage_out.cap & ~(size_t)3, &len, consumed, ix));
    *out_len = len;
    if (len > cap) return BZH_E_CAP;
    HIP_TRY(ctx, hipMemcpyAsync(out, ctx->d_stage_out, len, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, bzh_stream_wait(st));
    return BZH_OK;
}

extern "C" int bzh_encode(bzh_ctx *ctx, const uint8_t *in, size_t n, uint8_t *out, size_t cap, size_t *out_len,
                          size_t *consumed)
{
    return bzh_guard(ctx, [&]() -> int { return encode_host(ctx, in, n, out, cap, out_len, consumed, nullptr); });
}

// ---- the encoder writes the index of its own stream (sync_emit.hip) --------------------------------------------------------
extern "C" int bzh_encode_index_bound(int level, size_t n, uint32_t interval, size_t *max_entries, size_t *max_pts)
{
    if (level < 1 || level > 9 || interval > 32767 || !max_entries || !max_pts) return BZH_E_ARG;
    const size_t M = (size_t)100000 * level - 1;
    const size_t blocks = n / (M * 4 / 5) + 2;       // a block consumes at least M * 4 / 5 raw bytes (bzh_encode sizes its output so)
    const size_t groups = (M + 1 + 49) / 50;         // m <= M + 1 symbols (lib/mtf.rs:36), 50 a group
    *max_entries = blocks;
    *max_pts = interval ? blocks * ((groups - 1) / interval) : 0;
    return BZH_OK;
}

static int encode_index_args(bzh_ctx *ctx, uint32_t interval, bzh_index_entry *idx, size_t max, size_t *count, bzh_sync_point *pts,
                             size_t max_pts, size_t *npts)
{
    if (!ctx || !count || !npts || (!idx && max) || (!pts && max_pts)) return BZH_E_ARG;
    if (interval > 32767) {
        bzh_set_error(ctx, "encode index: a sync interval of %u groups, outside 0..32767", interval);
        return BZH_E_ARG;
    }
    *count = 0;
    *npts = 0;
    return BZH_OK;
}

static int encode_index_out(bzh_ctx *ctx, const EncIndex &ix, bzh_index_entry *idx, size_t max, size_t *count, bzh_sync_point *pts,
                            size_t max_pts, size_t *npts)
{
    *count = ix.entries.size();
    *npts = ix.pts.size();
    if (ix.entries.size() > max) {
        bzh_set_error(ctx, "encode index: %zu entries, room for %zu", ix.entries.size(), max);
        return BZH_E_CAP;
    }
    if (ix.pts.size() > max_pts) {
        bzh_set_error(ctx, "encode index: %zu sync points, room for %zu", ix.pts.size(), max_pts);
        return BZH_E_CAP;
    }
    if (!ix.entries.empty()) memcpy(idx, ix.entries.data(), ix.entries.size() * sizeof(bzh_index_entry));
    if (!ix.pts.empty()) memcpy(pts, ix.pts.data(), ix.pts.size() * sizeof(bzh_sync_point));
    return BZH_OK;
}

extern "C" int bzh_encode_index_device(bzh_ctx *ctx, const void *d_in, size_t n, void *d_out, size_t cap, size_t *out_len,
                                       size_t *consumed, uint32_t interval, bzh_index_entry *idx, size_t max, size_t *count,
                                       bzh_sync_point *pts, size_t max_pts, size_t *npts)
{
    return bzh_guard(ctx, [&]() -> int {
    BZH_TRY(encode_index_args(ctx, interval, idx, max, count, pts, max_pts, npts));
    EncIndex ix{interval, {}, {}};
    BZH_TRY(encode_device_impl(ctx, d_in, n, d_out, cap, out_len, consumed, &ix));
    return encode_index_out(ctx, ix, idx, max, count, pts, max_pts, npts);
    });
}

extern "C" int bzh_encode_index(bzh_ctx *ctx, const uint8_t *in, size_t n, uint8_t *out, size_t cap, size_t *out_len,
                                size_t *consumed, uint32_t interval, bzh_index_entry *idx, size_t max, size_t *count,
                                bzh_sync_point *pts, size_t max_pts, size_t *npts)
{
    return bzh_guard(ctx, [&]() -> int {
    BZH_TRY(encode_index_args(ctx, interval, idx, max, count, pts, max_pts, npts));
    EncIndex ix{interval, {}, {}};
    BZH_TRY(encode_host(ctx, in, n, out, cap, out_len, consumed, &ix));
    return encode_index_out(ctx, ix, idx, max, count, pts, max_pts, npts);
    });
}

// ---- stage seams: RLE1 split and CRC -------------------------------------------------------------------------
extern "C" int bzh_rle1_split(bzh_ctx *ctx, const uint8_t *in, size_t n, bzh_block *blocks, size_t max_blocks,
                              size_t *nblocks, uint8_t *rle_out, size_t rle_cap)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || (!in && n) || !blocks || !nblocks) return BZH_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    stats_begin(ctx);
    BZH_TRY(ensure_stage(ctx, ctx->d_stage_in, n + 16));
    if (n) HIP_TRY(ctx, hipMemcpyAsync(ctx->d_stage_in, in, n, hipMemcpyHostToDevice, st));
    BZH_TRY(rle1_plan(ctx, ctx->d_stage_in, n));
    const size_t nb = ctx->plan_blocks.size();
    *nblocks = nb;
    if (nb > max_blocks) return BZH_E_CAP;
    for (size_t k = 0; k < nb; k++) blocks[k] = ctx->plan_blocks[k];
    if (rle_out) {
        size_t pos = 0;
        BZH_TRY(ensure_arena(ctx, (uint32_t)std::min<size_t>(nb, ctx->max_batch)));
        Batch &bt = ctx->bt;
        for (size_t k0 = 0; k0 < nb; k0 += ctx->max_batch) {
            const uint32_t B = (uint32_t)std::min<size_t>(ctx->max_batch, nb - k0);
            BZH_TRY(rle1_emit(ctx, k0, B));
            for (uint32_t b = 0; b < B; b++) {
                const size_t len = ctx->plan_blocks[k0 + b].rle_len;
                if (pos + len > rle_cap) return BZH_E_CAP;
                HIP_TRY(ctx, hipMemcpyAsync(rle_out + pos, bt.rle + (size_t)b * bt.S, len, hipMemcpyDeviceToHost, st));
                pos += len;
            }
            HIP_TRY(ctx, bzh_stream_wait(st));
        }
    }
    return BZH_OK;
    });
}

extern "C" int bzh_crc32(bzh_ctx *ctx, const uint8_t *in, size_t n, uint32_t *crc)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || (!in && n) || !crc) return BZH_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    BZH_TRY(ensure_stage(ctx, ctx->d_stage_in, n + 16));
    if (n) HIP_TRY(ctx, hipMemcpyAsync(ctx->d_stage_in, in, n, hipMemcpyHostToDevice, ctx->stream));
    BZH_TRY(ensure_arena(ctx, 1)); // (crc_device borrows two words of it)
    return crc_device(ctx, ctx->d_stage_in, n, crc);
    });
}

// ================================================================================================
// Decode (decode.hip): scan, then the arena for as many blocks as there are candidates, then the chain
// ================================================================================================
// What every decode call does around its work: the device, fresh statistics, and with profiling on the events of the whole call
// and of its scan (a range has none).
struct DecodeCall {
    hipEvent_t t0 = nullptr, t1 = nullptr;
};

static int decode_call_begin(bzh_ctx *ctx, size_t n, DecodeCall &c)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ctx->evnext = 0;
    ctx->sort_spans.clear();
    kstats_reset(ctx);
    memset(&ctx->dstats, 0, sizeof ctx->dstats);
    ctx->dstats.in_bytes = n;
    c.t0 = call_mark(ctx);
    return BZH_OK;
}

// the scan, and the arena for as many blocks as it found candidates
static int decode_call_scan(bzh_ctx *ctx, DecodeCall &c, const void *d_in, size_t n, std::vector<uint64_t> &cands)
{
    BZH_TRY(decode_scan_run(ctx, (const uint8_t *)d_in, n, cands));
    c.t1 = call_mark(ctx);
    ctx->dstats.candidates = cands.size();
    return ensure_arena(ctx, (uint32_t)std::min<size_t>(std::max<size_t>(cands.size(), 1), ctx->max_batch));
}

// rc: the status of the work, handed through
static int decode_call_end(bzh_ctx *ctx, const DecodeCall &c, int rc)
{
    if (!ctx->profiling) return rc;
    hipEvent_t t2 = call_mark(ctx);
    HIP_TRY(ctx, bzh_stream_wait(ctx->stream));
    if (c.t1) ctx->dstats.ms_scan = span_ms(c.t0, c.t1);
    ctx->dstats.ms_total = span_ms(c.t0, t2);
    return rc;
}

// The host variants: the input into the staging buffer (queued), room for out_bytes of output in the other one.
static int decode_stage(bzh_ctx *ctx, const uint8_t *in, size_t n, size_t out_bytes = 0)
{
    BZH_TRY(ensure_stage(ctx, ctx->d_stage_in, n + 16));
    if (out_bytes) BZH_TRY(ensure_stage(ctx, ctx->d_stage_out, out_bytes));
    if (n) HIP_TRY(ctx, hipMemcpyAsync(ctx->d_stage_in, in, n, hipMemcpyHostToDevice, ctx->stream));
    return BZH_OK;
}

// decode_stage for the host variants of a read by index (range, ranges, records): of the caller's n bytes, which begin at byte
// in_byte_base of the indexed input, only the hull [lo, hi) of the touched blocks goes up.  A buffer that does not cover it goes up
// whole: the device call says what is missing.  *base, *un: where in the indexed input the staged bytes begin, and their number.
static int decode_stage_hull(bzh_ctx *ctx, const uint8_t *in, size_t n, uint64_t in_byte_base, uint64_t lo, uint64_t hi, size_t out_bytes,
                             uint64_t *base, size_t *un)
{
    const bool covered = lo <= hi && in_byte_base <= lo && hi - in_byte_base <= n;
    *base = covered ? lo : in_byte_base;
    *un = covered ? (size_t)(hi - lo) : n;
    return decode_stage(ctx, covered ? in + (lo - in_byte_base) : in, *un, out_bytes);
}

// ... and their tail: `len` bytes of the staged output to the caller's buffer, and the wait.
static int decode_unstage(bzh_ctx *ctx, uint8_t *out, size_t len)
{
    if (len) HIP_TRY(ctx, hipMemcpyAsync(out, ctx->d_stage_out, len, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, bzh_stream_wait(ctx->stream));
    return BZH_OK;
}

extern "C" int bzh_decode_device(bzh_ctx *ctx, const void *d_in, size_t n, void *d_out, size_t cap, size_t *out_len, size_t *consumed)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || (!d_in && n) || (!d_out && cap) || !out_len) return BZH_E_ARG;
    DecodeCall call;
    BZH_TRY(decode_call_begin(ctx, n, call));
    *out_len = 0;
    if (consumed) *consumed = 0;
    std::vector<uint64_t> cands;
    BZH_TRY(decode_call_scan(ctx, call, d_in, n, cands));
    const int rc = decode_chain_run(ctx, (const uint8_t *)d_in, n, (uint8_t *)d_out, cap, out_len, consumed, cands);
    return decode_call_end(ctx, call, rc);
    });
}

extern "C" int bzh_decode(bzh_ctx *ctx, const uint8_t *in, size_t n, uint8_t *out, size_t cap, size_t *out_len, size_t *consumed)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || (!in && n) || (!out && cap) || !out_len) return BZH_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    BZH_TRY(decode_stage(ctx, in, n, cap));
    size_t len = 0;
    const int rc = bzh_decode_device(ctx, ctx->d_stage_in, n, cap ? ctx->d_stage_out : nullptr, cap, &len, consumed);
    *out_len = len; // (BZH_E_CAP: the size needed)
    if (rc != BZH_OK) return rc;
    if (len) HIP_TRY(ctx, hipMemcpyAsync(out, ctx->d_stage_out, len, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, bzh_stream_wait(ctx->stream));
    return BZH_OK;
    });
}

// ---- streaming decode (decode.hip's dstream_*; the walk and the feed loop: decode_stream_plan.h) ----
static int dstream_arena(bzh_ctx *ctx, uint32_t blocks) { return ensure_arena(ctx, blocks); }

extern "C" int bzh_dstream_set_room(bzh_ctx *ctx, size_t window_bytes, size_t staging_bytes)
{
    return bzh_guard(ctx, [&]() -> int {
    if (!ctx) return BZH_E_ARG;
    if ((window_bytes && window_bytes < 1024) || (staging_bytes && staging_bytes < 1024)) {
        bzh_set_error(ctx, "dstream: a room of %zu / %zu bytes, below 1024", window_bytes, staging_bytes);
        return BZH_E_ARG;
    }
    ctx->dstrm_window = window_bytes;
    ctx->dstrm_staging = staging_bytes;
    return BZH_OK;
    });
}

extern "C" int bzh_dstream_begin(bzh_ctx *ctx)
{
    return bzh_guard(ctx, [&]() -> int {
    if (!ctx) return BZH_E_ARG;
    stream_join(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return dstream_begin(ctx);
    });
}

extern "C" int bzh_dstream_feed(bzh_ctx *ctx, const uint8_t *in, size_t n, int eof, size_t *in_used, uint8_t *out, size_t cap, size_t *out_len,
                                int *done)
{
    return bzh_guard(ctx, [&]() -> int {
    if (!ctx || (!in && n) || (!out && cap) || !in_used || !out_len || !done) return BZH_E_ARG;
    stream_join(ctx);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return dstream_feed(ctx, dstream_arena, in, n, eof, in_used, out, cap, out_len, done);
    });
}

extern "C" size_t bzh_dstream_consumed(const bzh_ctx *ctx) { return ctx ? dstream_consumed(ctx) : 0; }

extern "C" int bzh_dstream_get_stats(const bzh_ctx *ctx, bzh_dstream_stats *out)
{
    return bzh_guard(const_cast<bzh_ctx *>(ctx), [&]() -> int {
    if (!ctx || !out) return BZH_E_ARG;
    return dstream_stats(ctx, out);
    });
}

extern "C" int bzh_dstream_end(bzh_ctx *ctx)
{
    return bzh_guard(ctx, [&]() -> int {
    if (!ctx) return BZH_E_ARG;
    dstream_end(ctx);
    return BZH_OK;
    });
}

// ---- random access (decode.hip): the index is bzh_decode_device's flow with no output, a range needs neither scan nor chain
// interval 0: no sync points (bzh_decode_index_device); else bzh_decode_index_sync_device
// rec: also the record table (bzh_decode_index_records_device)
struct RecOut {
    uint8_t delim;
    uint64_t *rec_cum;
    size_t max_cum;
    uint64_t *nrecords;
};
static int decode_index_device_impl(bzh_ctx *ctx, const void *d_in, size_t n, uint32_t interval, bzh_index_entry *idx, size_t max, size_t *count,
                                    bzh_sync_point *pts, size_t max_pts, size_t *npts, uint64_t *out_total, size_t *consumed,
                                    const RecOut *rec = nullptr)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || (!d_in && n) || (!idx && max) || !count || !out_total || (!pts && max_pts) || (interval && !npts)) return BZH_E_ARG;
    DecodeCall call;
    BZH_TRY(decode_call_begin(ctx, n, call));
    *count = 0;
    *out_total = 0;
    if (npts) *npts = 0;
    if (consumed) *consumed = 0;
    std::vector<uint64_t> cands;
    BZH_TRY(decode_call_scan(ctx, call, d_in, n, cands));
    std::vector<bzh_index_entry> entries;
    size_t total = 0;
    SyncBuild sync{interval, {}};
    RecBuild rb{rec ? rec->delim : 0u, {}, false};
    if (rec) *rec->nrecords = 0;
    int rc = decode_chain_run(ctx, (const uint8_t *)d_in, n, nullptr, 0, &total, consumed, cands, &entries, interval ? &sync : nullptr,
                              rec ? &rb : nullptr);
    rc = decode_call_end(ctx, call, rc);
    if (rc != BZH_OK) return rc;
    *count = entries.size();
    *out_total = total;
    if (npts) *npts = sync.pts.size();
    if (entries.size() > max) {
        bzh_set_error(ctx, "decode index: %zu entries, room for %zu", entries.size(), max);
        return BZH_E_CAP;
    }
    if (sync.pts.size() > max_pts) {
        bzh_set_error(ctx, "decode index: %zu sync points, room for %zu", sync.pts.size(), max_pts);
        return BZH_E_CAP;
    }
    if (rec && entries.size() + 1 > rec->max_cum) {
        bzh_set_error(ctx, "decode index: a record table of %zu words, room for %zu", entries.size() + 1, rec->max_cum);
        return BZH_E_CAP;
    }
    if (!entries.empty()) memcpy(idx, entries.data(), entries.size() * sizeof(bzh_index_entry));
    if (!sync.pts.empty()) memcpy(pts, sync.pts.data(), sync.pts.size() * sizeof(bzh_sync_point));
    if (rec) {
        memcpy(rec->rec_cum, rb.cum.data(), rb.cum.size() * sizeof(uint64_t));
        *rec->nrecords = rb.cum.back() + (total > 0 && !rb.last_is_delim);
    }
    return BZH_OK;
    });
}

extern "C" int bzh_decode_index_device(bzh_ctx *ctx, const void *d_in, size_t n, bzh_index_entry *idx, size_t max, size_t *count,
                                       uint64_t *out_total, size_t *consumed)
{
    return decode_index_device_impl(ctx, d_in, n, 0, idx, max, count, nullptr, 0, nullptr, out_total, consumed);
}

static bool sync_interval_ok(bzh_ctx *ctx, uint32_t interval)
{
    if (interval >= 1 && interval <= 32767) return true;
    if (ctx) bzh_set_error(ctx, "decode index: a sync interval of %u groups, outside 1..32767", interval);
    return false;
}

extern "C" int bzh_decode_index_sync_device(bzh_ctx *ctx, const void *d_in, size_t n, uint32_t interval, bzh_index_entry *idx, size_t max,
                                            size_t *count, bzh_sync_point *pts, size_t max_pts, size_t *npts, uint64_t *out_total,
                                            size_t *consumed)
{
    if (!ctx || !npts) return BZH_E_ARG;
    if (!sync_interval_ok(ctx, interval)) return BZH_E_ARG;
    return decode_index_device_impl(ctx, d_in, n, interval, idx, max, count, pts, max_pts, npts, out_total, consumed);
}

extern "C" int bzh_decode_index_sync(bzh_ctx *ctx, const uint8_t *in, size_t n, uint32_t interval, bzh_index_entry *idx, size_t max,
                                     size_t *count, bzh_sync_point *pts, size_t max_pts, size_t *npts, uint64_t *out_total, size_t *consumed)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || (!in && n) || (!idx && max) || !count || !out_total || (!pts && max_pts) || !npts) return BZH_E_ARG;
    if (!sync_interval_ok(ctx, interval)) return BZH_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    BZH_TRY(decode_stage(ctx, in, n));
    return decode_index_device_impl(ctx, ctx->d_stage_in, n, interval, idx, max, count, pts, max_pts, npts, out_total, consumed);
    });
}

extern "C" int bzh_decode_index(bzh_ctx *ctx, const uint8_t *in, size_t n, bzh_index_entry *idx, size_t max, size_t *count,
                                uint64_t *out_total, size_t *consumed)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || (!in && n) || (!idx && max) || !count || !out_total) return BZH_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    BZH_TRY(decode_stage(ctx, in, n));
    return bzh_decode_index_device(ctx, ctx->d_stage_in, n, idx, max, count, out_total, consumed);
    });
}

// npts 0: bzh_decode_range_device; else bzh_decode_range_sync_device
static int decode_range_device_impl(bzh_ctx *ctx, const void *d_in, size_t n, uint64_t in_byte_base, const bzh_index_entry *idx, size_t count,
                                    const bzh_sync_point *pts, size_t npts, uint64_t off, uint64_t len, void *d_out, size_t cap,
                                    size_t *out_len)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || (!d_in && n) || (!d_out && cap) || (!idx && count) || (!pts && npts) || !out_len) return BZH_E_ARG;
    DecodeCall call;
    BZH_TRY(decode_call_begin(ctx, n, call));
    *out_len = 0;
    if (count > 0xFFFFFFFFull) { // (the front numbers the entries of a batch in 32 bits, as a sync point does its own)
        bzh_set_error(ctx, "decode range: an index of %zu entries, 2^32 or more", count);
        return BZH_E_ARG;
    }
    BZH_TRY(decode_index_check(ctx, idx, count)); // (before any arithmetic on the entries)
    BZH_TRY(decode_sync_check(ctx, idx, count, pts, npts));
    size_t first = 0, last = 0;
    uint64_t lo, hi;
    BZH_TRY(bzh_index_span(idx, count, off, len, &first, &last, &lo, &hi));
    BZH_TRY(ensure_arena(ctx, (uint32_t)std::min<size_t>(std::max<size_t>(last - first, 1), ctx->max_batch)));
    const int rc = decode_range_run(ctx, (const uint8_t *)d_in, n, in_byte_base, idx, count, off, len, (uint8_t *)d_out, cap, out_len, pts,
                                     npts);
    return decode_call_end(ctx, call, rc);
    });
}

extern "C" int bzh_decode_range_device(bzh_ctx *ctx, const void *d_in, size_t n, uint64_t in_byte_base, const bzh_index_entry *idx,
                                       size_t count, uint64_t off, uint64_t len, void *d_out, size_t cap, size_t *out_len)
{
    return decode_range_device_impl(ctx, d_in, n, in_byte_base, idx, count, nullptr, 0, off, len, d_out, cap, out_len);
}

extern "C" int bzh_decode_range_sync_device(bzh_ctx *ctx, const void *d_in, size_t n, uint64_t in_byte_base, const bzh_index_entry *idx,
                                            size_t count, const bzh_sync_point *pts, size_t npts, uint64_t off, uint64_t len, void *d_out,
                                            size_t cap, size_t *out_len)
{
    return decode_range_device_impl(ctx, d_in, n, in_byte_base, idx, count, pts, npts, off, len, d_out, cap, out_len);
}

static int decode_range_impl(bzh_ctx *ctx, const uint8_t *in, size_t n, uint64_t in_byte_base, const bzh_index_entry *idx, size_t count,
                             const bzh_sync_point *pts, size_t npts, uint64_t off, uint64_t len, uint8_t *out, size_t cap, size_t *out_len)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || (!in && n) || (!out && cap) || (!idx && count) || (!pts && npts) || !out_len) return BZH_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    *out_len = 0;
    BZH_TRY(decode_index_check(ctx, idx, count)); // (before any arithmetic on the entries)
    BZH_TRY(decode_sync_check(ctx, idx, count, pts, npts));
    // only the span goes up
    size_t first = 0, last = 0;
    uint64_t lo = 0, hi = 0;
    BZH_TRY(bzh_index_span(idx, count, off, len, &first, &last, &lo, &hi));
    const uint64_t total = count ? idx[count - 1].out_off + idx[count - 1].out_len : 0;
    const uint64_t want = off < total ? std::min<uint64_t>(len, total - off) : 0;
    if (want > cap) {
        bzh_set_error(ctx, "decode range: the range holds %llu bytes, the buffer %zu", (unsigned long long)want, cap);
        return BZH_E_ARG;
    }
    uint64_t base;
    size_t un, got = 0;
    BZH_TRY(decode_stage_hull(ctx, in, n, in_byte_base, lo, hi, (size_t)want, &base, &un));
    BZH_TRY(decode_range_device_impl(ctx, ctx->d_stage_in, un, base, idx, count, pts, npts, off, len, want ? ctx->d_stage_out : nullptr,
                                     (size_t)want, &got));
    BZH_TRY(decode_unstage(ctx, out, got));
    *out_len = got;
    return BZH_OK;
    });
}

extern "C" int bzh_decode_range(bzh_ctx *ctx, const uint8_t *in, size_t n, uint64_t in_byte_base, const bzh_index_entry *idx, size_t count,
                                uint64_t off, uint64_t len, uint8_t *out, size_t cap, size_t *out_len)
{
    return decode_range_impl(ctx, in, n, in_byte_base, idx, count, nullptr, 0, off, len, out, cap, out_len);
}

extern "C" int bzh_decode_range_sync(bzh_ctx *ctx, const uint8_t *in, size_t n, uint64_t in_byte_base, const bzh_index_entry *idx,
                                     size_t count, const bzh_sync_point *pts, size_t npts, uint64_t off, uint64_t len, uint8_t *out,
                                     size_t cap, size_t *out_len)
{
    return decode_range_impl(ctx, in, n, in_byte_base, idx, count, pts, npts, off, len, out, cap, out_len);
}

// ---- many ranges (decode.hip's decode_ranges_run; the arithmetic: decode_plan.h)
extern "C" int bzh_decode_ranges_device(bzh_ctx *ctx, const void *d_in, size_t n, uint64_t in_byte_base, const bzh_index_entry *idx,
                                        size_t count, const bzh_sync_point *pts, size_t npts, const bzh_range *ranges, size_t nranges,
                                        void *d_out, size_t cap, size_t *out_offs, size_t *out_lens, size_t *out_total)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || (!d_in && n) || (!d_out && cap) || (!idx && count) || (!pts && npts) || (!ranges && nranges) || (!out_offs && nranges) ||
        (!out_lens && nranges) || !out_total)
        return BZH_E_ARG;
    DecodeCall call;
    BZH_TRY(decode_call_begin(ctx, n, call));
    memset(&ctx->qstats, 0, sizeof ctx->qstats);
    // where the bytes go: arithmetic that stays inside the arrays whatever they hold, so it comes before the checks and holds on
    // every error behind this line
    std::vector<uint32_t> touched;
    uint64_t lo = 0, hi = 0;
    const uint64_t total = count <= 0xFFFFFFFFull ? bzp_spans(idx, count, ranges, nranges, out_offs, out_lens, touched, &lo, &hi)
                                                  : bzp_spans(idx, 0, ranges, nranges, out_offs, out_lens, touched, &lo, &hi);
    *out_total = (size_t)total;
    if (count > 0xFFFFFFFFull) {
        bzh_set_error(ctx, "decode ranges: an index of %zu entries, 2^32 or more", count);
        return BZH_E_ARG;
    }
    BZH_TRY(decode_index_check(ctx, idx, count));
    BZH_TRY(decode_sync_check(ctx, idx, count, pts, npts));
    ctx->qstats.ranges = nranges;
    ctx->qstats.blocks_touched = touched.size();
    if (total > cap) {
        bzh_set_error(ctx, "decode ranges: the ranges hold %llu bytes, the buffer %zu", (unsigned long long)total, cap);
        return BZH_E_CAP;
    }
    BZH_TRY(ensure_arena(ctx, (uint32_t)std::min<size_t>(std::max<size_t>(touched.size(), 1), ctx->max_batch)));
    const int rc = decode_ranges_run(ctx, (const uint8_t *)d_in, n, in_byte_base, idx, count, pts, npts, ranges, nranges, out_offs, touched,
                                     (uint8_t *)d_out, total);
    return decode_call_end(ctx, call, rc);
    });
}

extern "C" int bzh_decode_ranges(bzh_ctx *ctx, const uint8_t *in, size_t n, uint64_t in_byte_base, const bzh_index_entry *idx, size_t count,
                                 const bzh_sync_point *pts, size_t npts, const bzh_range *ranges, size_t nranges, uint8_t *out, size_t cap,
                                 size_t *out_offs, size_t *out_lens, size_t *out_total)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || (!in && n) || (!out && cap) || (!idx && count) || (!pts && npts) || (!ranges && nranges) || (!out_offs && nranges) ||
        (!out_lens && nranges) || !out_total)
        return BZH_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // only the hull goes up
    uint64_t lo = 0, hi = 0, total = 0;
    if (count <= 0xFFFFFFFFull) {
        std::vector<uint32_t> touched;
        total = bzp_spans(idx, count, ranges, nranges, nullptr, nullptr, touched, &lo, &hi);
    }
    const size_t room = total <= cap ? (size_t)total : 0; // (too small: the device call sets the sizes and says so)
    uint64_t base;
    size_t un;
    BZH_TRY(decode_stage_hull(ctx, in, n, in_byte_base, lo, hi, room, &base, &un));
    BZH_TRY(bzh_decode_ranges_device(ctx, ctx->d_stage_in, un, base, idx, count, pts, npts, ranges, nranges,
                                     room ? ctx->d_stage_out : nullptr, room, out_offs, out_lens, out_total));
    return decode_unstage(ctx, out, *out_total);
    });
}

// ---- records (decode.hip: the count in the chain walk, decode_records_run, count_records_run; the arithmetic: decode_records_plan.h)
extern "C" int bzh_decode_index_records_device(bzh_ctx *ctx, const void *d_in, size_t n, uint32_t interval, uint8_t delim, bzh_index_entry *idx,
                                               size_t max, size_t *count, bzh_sync_point *pts, size_t max_pts, size_t *npts, uint64_t *rec_cum,
                                               size_t max_cum, uint64_t *nrecords, uint64_t *out_total, size_t *consumed)
{
    if (!ctx || !npts || !nrecords || (!rec_cum && max_cum)) return BZH_E_ARG;
    if (interval && !sync_interval_ok(ctx, interval)) return BZH_E_ARG;
    const RecOut rec{delim, rec_cum, max_cum, nrecords};
    return decode_index_device_impl(ctx, d_in, n, interval, idx, max, count, pts, max_pts, npts, out_total, consumed, &rec);
}

extern "C" int bzh_decode_index_records(bzh_ctx *ctx, const uint8_t *in, size_t n, uint32_t interval, uint8_t delim, bzh_index_entry *idx,
                                        size_t max, size_t *count, bzh_sync_point *pts, size_t max_pts, size_t *npts, uint64_t *rec_cum,
                                        size_t max_cum, uint64_t *nrecords, uint64_t *out_total, size_t *consumed)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || (!in && n) || (!idx && max) || !count || !out_total || (!pts && max_pts) || !npts || !nrecords || (!rec_cum && max_cum))
        return BZH_E_ARG;
    if (interval && !sync_interval_ok(ctx, interval)) return BZH_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    BZH_TRY(decode_stage(ctx, in, n));
    return bzh_decode_index_records_device(ctx, ctx->d_stage_in, n, interval, delim, idx, max, count, pts, max_pts, npts, rec_cum, max_cum,
                                           nrecords, out_total, consumed);
    });
}

extern "C" int bzh_count_records_device(bzh_ctx *ctx, const void *d_raw, size_t n, uint8_t delim, const bzh_index_entry *idx, size_t count,
                                        uint64_t *rec_cum, uint64_t *nrecords)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || (!d_raw && n) || (!idx && count) || !rec_cum || !nrecords) return BZH_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (count > 0xFFFFFFFFull) {
        bzh_set_error(ctx, "count records: an index of %zu entries, 2^32 or more", count);
        return BZH_E_ARG;
    }
    BZH_TRY(decode_index_check(ctx, idx, count));
    const uint64_t total = count ? idx[count - 1].out_off + idx[count - 1].out_len : 0;
    if (total != n) {
        bzh_set_error(ctx, "count records: the index holds %llu bytes, the buffer %zu", (unsigned long long)total, n);
        return BZH_E_ARG;
    }
    return count_records_run(ctx, (const uint8_t *)d_raw, n, delim, idx, count, rec_cum, nrecords);
    });
}

// the checks both variants make before any arithmetic on the arrays; the touched entries
static int decode_records_args(bzh_ctx *ctx, const bzh_index_entry *idx, size_t count, const bzh_sync_point *pts, size_t npts,
                               const uint64_t *rec_cum, const bzh_range *ranges, size_t nranges, std::vector<uint32_t> &touched, uint64_t *lo,
                               uint64_t *hi)
{
    if (count > 0xFFFFFFFFull) {
        bzh_set_error(ctx, "decode records: an index of %zu entries, 2^32 or more", count);
        return BZH_E_ARG;
    }
    BZH_TRY(decode_index_check(ctx, idx, count));
    BZH_TRY(decode_sync_check(ctx, idx, count, pts, npts));
    size_t bad = 0;
    if (const char *what = bzq_table_check(idx, count, rec_cum, &bad)) {
        bzh_set_error(ctx, "decode records: record table, entry %zu: %s", bad, what);
        return BZH_E_ARG;
    }
    bzq_spans(idx, count, rec_cum, ranges, nranges, touched, lo, hi);
    return BZH_OK;
}

extern "C" int bzh_decode_records_device(bzh_ctx *ctx, const void *d_in, size_t n, uint64_t in_byte_base, const bzh_index_entry *idx,
                                         size_t count, const bzh_sync_point *pts, size_t npts, const uint64_t *rec_cum, uint8_t delim,
                                         const bzh_range *ranges, size_t nranges, void *d_out, size_t cap, size_t *out_offs, size_t *out_lens,
                                         size_t *out_total)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || (!d_in && n) || (!d_out && cap) || (!idx && count) || (!pts && npts) || !rec_cum || (!ranges && nranges) ||
        (!out_offs && nranges) || (!out_lens && nranges) || !out_total)
        return BZH_E_ARG;
    DecodeCall call;
    BZH_TRY(decode_call_begin(ctx, n, call));
    memset(&ctx->qstats, 0, sizeof ctx->qstats);
    *out_total = 0;
    for (size_t r = 0; r < nranges; r++) out_offs[r] = out_lens[r] = 0;
    std::vector<uint32_t> touched;
    uint64_t lo = 0, hi = 0;
    BZH_TRY(decode_records_args(ctx, idx, count, pts, npts, rec_cum, ranges, nranges, touched, &lo, &hi));
    ctx->qstats.ranges = nranges;
    ctx->qstats.blocks_touched = touched.size();
    BZH_TRY(ensure_arena(ctx, (uint32_t)std::min<size_t>(std::max<size_t>(touched.size(), 1), ctx->max_batch)));
    const int rc = decode_records_run(ctx, (const uint8_t *)d_in, n, in_byte_base, idx, count, pts, npts, rec_cum, delim, ranges, nranges, touched,
                                      (uint8_t *)d_out, cap, out_offs, out_lens, out_total);
    return decode_call_end(ctx, call, rc);
    });
}

extern "C" int bzh_decode_records(bzh_ctx *ctx, const uint8_t *in, size_t n, uint64_t in_byte_base, const bzh_index_entry *idx, size_t count,
                                  const bzh_sync_point *pts, size_t npts, const uint64_t *rec_cum, uint8_t delim, const bzh_range *ranges,
                                  size_t nranges, uint8_t *out, size_t cap, size_t *out_offs, size_t *out_lens, size_t *out_total)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || (!in && n) || (!out && cap) || (!idx && count) || (!pts && npts) || !rec_cum || (!ranges && nranges) ||
        (!out_offs && nranges) || (!out_lens && nranges) || !out_total)
        return BZH_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    *out_total = 0;
    // only the hull goes up
    std::vector<uint32_t> touched;
    uint64_t lo = 0, hi = 0;
    BZH_TRY(decode_records_args(ctx, idx, count, pts, npts, rec_cum, ranges, nranges, touched, &lo, &hi));
    uint64_t base;
    size_t un;
    BZH_TRY(decode_stage_hull(ctx, in, n, in_byte_base, lo, hi, cap, &base, &un));
    BZH_TRY(bzh_decode_records_device(ctx, ctx->d_stage_in, un, base, idx, count, pts, npts, rec_cum, delim, ranges, nranges,
                                      cap ? ctx->d_stage_out : nullptr, cap, out_offs, out_lens, out_total));
    return decode_unstage(ctx, out, *out_total);
    });
}

// ---- search, grep, match (search.hip, grep.hip, match.hip: the kernels, the passes over a window, the staging and the carry,
// each as a ScanSink: common.h; the windows: search_plan.h, grep_plan.h, match_plan.h).  Five routes take decoded or compressed
// bytes to a sink, whichever it is: decoded bytes in HBM, the full decode (decode_chain_run) and the indexed one
// (decode_range_sink_run) from the device, and the latter two from the host.  A family is a sink type and a ScanFamily; every
// public call makes its sink and names its route.
struct ScanFamily {
    const char *name;      // in the messages
    unsigned flag;         // the one flag it defines
    const char *flag_name;
    bool bytes;            // it writes bytes: out_total belongs to every call, the output buffer is 4-byte aligned
    void (*clear)(bzh_ctx *); // the statistics of its last call
};
static void search_stats_clear(bzh_ctx *c) { memset(&c->sstats, 0, sizeof c->sstats); }
static void grep_stats_clear(bzh_ctx *c) { memset(&c->gstats, 0, sizeof c->gstats), memset(&c->gcstats, 0, sizeof c->gcstats); }
static void match_stats_clear(bzh_ctx *c) { memset(&c->mtstats, 0, sizeof c->mtstats); }
static const ScanFamily SEARCH = {"search", BZH_SEARCH_RECORDS, "BZH_SEARCH_RECORDS", false, search_stats_clear};
static const ScanFamily GREP = {"grep", BZH_GREP_INVERT, "BZH_GREP_INVERT", true, grep_stats_clear};
static const ScanFamily MATCH = {"match", BZH_MATCH_RECORDS, "BZH_MATCH_RECORDS", true, match_stats_clear};
static ScanWhat what_pat(const uint8_t *pat, size_t plen) { return ScanWhat{pat, plen, nullptr, false}; }
static ScanWhat what_set(const bzh_patset *set) { return ScanWhat{nullptr, 0, set, true}; }

// The checks every call makes first, in this order: the pointers (nothing has been written yet), then the caller's counts are
// zeroed, then the pattern's length or the device of a set, the flags, the alignment of the output.  Behind them the statistics
// are fresh and the sink is armed.
static int scan_begin(bzh_ctx *ctx, const ScanFamily &f, ScanSink &s, size_t *count, uint64_t *out_total)
{
    const ScanArgs &a = s.args;
    if (!a.what.given() || !count || (f.bytes && !out_total) || (!a.out && a.cap) || (!a.ent && a.max)) return BZH_E_ARG;
    *count = 0;
    if (out_total) *out_total = 0;
    if (a.what.is_set && a.what.set->device != ctx->device) {
        bzh_set_error(ctx, "%s: the pattern set lies on device %d, the context on device %d", f.name, a.what.set->device, ctx->device);
        return BZH_E_ARG;
    }
    if (!a.what.is_set && (a.what.plen == 0 || a.what.plen > BZH_SEARCH_MAX_PATTERN)) {
        bzh_set_error(ctx, "%s: a pattern of %zu bytes, outside 1..%d", f.name, a.what.plen, BZH_SEARCH_MAX_PATTERN);
        return BZH_E_ARG;
    }
    if (a.flags & ~f.flag) {
        bzh_set_error(ctx, "%s: flags 0x%x, of which only %s is defined", f.name, a.flags, f.flag_name);
        return BZH_E_ARG;
    }
    if (f.bytes && ((uintptr_t)a.out & 3u)) {
        bzh_set_error(ctx, "%s: the output buffer is not 4-byte aligned", f.name);
        return BZH_E_ARG;
    }
    f.clear(ctx);
    s.arm(ctx);
    return BZH_OK;
}

// rc: the status of the windows.  Behind them what the sink held back; hits, bytes and entries follow the stream: whatever the
// status, nothing is on its way to the caller's arrays when the call returns.
static int scan_end(bzh_ctx *ctx, ScanSink &s, const DecodeCall &call, int rc, size_t *count, uint64_t *out_total)
{
    if (rc == BZH_OK) rc = s.finish(ctx);
    rc = decode_call_end(ctx, call, rc);
    HIP_TRY(ctx, bzh_stream_wait(ctx->stream));
    if (rc != BZH_OK) return rc;
    return s.report(ctx, count, out_total);
}

static int scan_raw_device(bzh_ctx *ctx, const ScanFamily &f, ScanSink &s, const void *d_raw, size_t n, size_t *count, uint64_t *out_total)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || (!d_raw && n)) return BZH_E_ARG;
    BZH_TRY(scan_begin(ctx, f, s, count, out_total));
    if ((uintptr_t)d_raw & 15u) {
        bzh_set_error(ctx, "%s: the buffer is not 16-byte aligned", f.name);
        return BZH_E_ARG;
    }
    DecodeCall call;
    BZH_TRY(decode_call_begin(ctx, n, call));
    const int rc = s.raw(ctx, (const uint8_t *)d_raw, n);
    return scan_end(ctx, s, call, rc, count, out_total);
    });
}

static int scan_device(bzh_ctx *ctx, const ScanFamily &f, ScanSink &s, const void *d_in, size_t n, size_t *count, uint64_t *out_total,
                       uint64_t *decoded_total, size_t *consumed)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || (!d_in && n)) return BZH_E_ARG;
    BZH_TRY(scan_begin(ctx, f, s, count, out_total));
    DecodeCall call;
    BZH_TRY(decode_call_begin(ctx, n, call));
    if (decoded_total) *decoded_total = 0;
    if (consumed) *consumed = 0;
    std::vector<uint64_t> cands;
    BZH_TRY(decode_call_scan(ctx, call, d_in, n, cands));
    size_t total = 0;
    const int rc = decode_chain_run(ctx, (const uint8_t *)d_in, n, nullptr, 0, &total, consumed, cands, nullptr, nullptr, nullptr, &s);
    if (decoded_total) *decoded_total = total;
    return scan_end(ctx, s, call, rc, count, out_total);
    });
}

// the host variants: room for the bytes in the staging buffer of the output (asked for with no room: a buffer all the same)
static size_t scan_stage_room(const void *out, size_t cap) { return out ? std::max<size_t>(cap, 16) : 0; }

// ... the sink's output moves to it, and the bytes come back only behind BZH_OK
static int scan_host(bzh_ctx *ctx, const ScanFamily &f, ScanSink &s, const uint8_t *in, size_t n, size_t *count, uint64_t *out_total,
                     uint64_t *decoded_total, size_t *consumed)
{
    return bzh_guard(ctx, [&]() -> int {
    uint8_t *const out = (uint8_t *)s.args.out;
    if (ctx) stream_join(ctx);
    if (!ctx || (!in && n) || (!out && s.args.cap)) return BZH_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    BZH_TRY(decode_stage(ctx, in, n, scan_stage_room(out, s.args.cap)));
    s.args.out = out ? ctx->d_stage_out.p : nullptr;
    BZH_TRY(scan_device(ctx, f, s, ctx->d_stage_in, n, count, out_total, decoded_total, consumed));
    return f.bytes ? decode_unstage(ctx, out, out ? (size_t)*out_total : 0) : BZH_OK;
    });
}

// the checks both variants of an indexed call make before any arithmetic on the arrays (flags: BZH_SEARCH_RECORDS asks for the table)
static int search_range_args(bzh_ctx *ctx, const bzh_index_entry *idx, size_t count, const bzh_sync_point *pts, size_t npts,
                             const uint64_t *rec_cum, unsigned flags)
{
    if (count > 0xFFFFFFFFull) {
        bzh_set_error(ctx, "search range: an index of %zu entries, 2^32 or more", count);
        return BZH_E_ARG;
    }
    BZH_TRY(decode_index_check(ctx, idx, count));
    BZH_TRY(decode_sync_check(ctx, idx, count, pts, npts));
    if (!(flags & BZH_SEARCH_RECORDS)) return BZH_OK;
    if (!rec_cum) {
        bzh_set_error(ctx, "search range: record numbers are asked for and no record table is given");
        return BZH_E_ARG;
    }
    size_t bad = 0;
    if (const char *what = bzq_table_check(idx, count, rec_cum, &bad)) {
        bzh_set_error(ctx, "search range: record table, entry %zu: %s", bad, what);
        return BZH_E_ARG;
    }
    return BZH_OK;
}

// The part of the output an indexed call is about, with the record table that numbers its records: a range search's.  The indexed
// grep and match take the whole output and no table: null.
struct ScanRange {
    uint64_t in_byte_base;
    const uint64_t *rec_cum;
    uint64_t off, len;
};

// The blocks a range search DECODES, and the bytes of the input that hold them: those of the wanted range, widened by the bytes an
// automaton with assertions looks at in front of it and behind it (decode_range_sink_run widens alike, and clips to the output);
// the hits stay inside the wanted range.
static int scan_range_span(const ScanWhat &q, const ScanRange &r, const bzh_index_entry *idx, size_t count, size_t *blocks, uint64_t *lo,
                           uint64_t *hi)
{
    uint64_t w_off = r.off, w_len = r.len;
    if (q.is_set && q.set->looks()) {
        const uint64_t back = std::min<uint64_t>(r.off, q.set->look.look_behind), more = back + q.set->look.look_ahead;
        w_off = r.off - back;
        w_len = r.len > ~0ull - more ? ~0ull : r.len + more;
    }
    size_t first = 0, last = 0;
    BZH_TRY(bzh_index_span(idx, count, w_off, w_len, &first, &last, lo, hi));
    *blocks = last - first;
    return BZH_OK;
}

static int scan_index_device(bzh_ctx *ctx, const ScanFamily &f, ScanSink &s, const void *d_in, size_t n, const bzh_index_entry *idx,
                             size_t count, const bzh_sync_point *pts, size_t npts, const ScanRange *range, size_t *found, uint64_t *out_total)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || (!d_in && n) || (!idx && count) || (!pts && npts)) return BZH_E_ARG;
    BZH_TRY(scan_begin(ctx, f, s, found, out_total));
    DecodeCall call;
    BZH_TRY(decode_call_begin(ctx, n, call));
    static const ScanRange whole = {0, nullptr, 0, ~0ull};
    const ScanRange &r = range ? *range : whole;
    const unsigned records = range ? s.args.flags & BZH_SEARCH_RECORDS : 0;
    BZH_TRY(search_range_args(ctx, idx, count, pts, npts, r.rec_cum, records));
    size_t blocks = count; // the arena: for the blocks of the range, or of the index
    uint64_t lo, hi;
    if (range) BZH_TRY(scan_range_span(s.args.what, r, idx, count, &blocks, &lo, &hi));
    BZH_TRY(ensure_arena(ctx, (uint32_t)std::min<size_t>(std::max<size_t>(blocks, 1), ctx->max_batch)));
    const int rc = decode_range_sink_run(ctx, (const uint8_t *)d_in, n, r.in_byte_base, idx, count, pts, npts, records ? r.rec_cum : nullptr,
                                         r.off, r.len, s);
    return scan_end(ctx, s, call, rc, found, out_total);
    });
}

// Of a range only the hull of its blocks goes up, so its arguments are checked here too: nothing goes up for a call that is
// refused.  Without a range the whole input goes up, as in scan_host.
static int scan_index_host(bzh_ctx *ctx, const ScanFamily &f, ScanSink &s, const uint8_t *in, size_t n, const bzh_index_entry *idx, size_t count,
                           const bzh_sync_point *pts, size_t npts, const ScanRange *range, size_t *found, uint64_t *out_total)
{
    return bzh_guard(ctx, [&]() -> int {
    uint8_t *const out = (uint8_t *)s.args.out;
    if (ctx) stream_join(ctx);
    if (!ctx || (!in && n) || (!idx && count) || (!pts && npts) || (!out && s.args.cap)) return BZH_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (range) {
        BZH_TRY(scan_begin(ctx, f, s, found, out_total));
        BZH_TRY(search_range_args(ctx, idx, count, pts, npts, range->rec_cum, s.args.flags));
        size_t blocks, un;
        uint64_t lo = 0, hi = 0;
        BZH_TRY(scan_range_span(s.args.what, *range, idx, count, &blocks, &lo, &hi)); // (the widened span: what the device variant is to be handed)
        ScanRange staged = *range;
        BZH_TRY(decode_stage_hull(ctx, in, n, range->in_byte_base, lo, hi, 0, &staged.in_byte_base, &un));
        return scan_index_device(ctx, f, s, ctx->d_stage_in, un, idx, count, pts, npts, &staged, found, out_total);
    }
    BZH_TRY(decode_stage(ctx, in, n, scan_stage_room(out, s.args.cap)));
    s.args.out = out ? ctx->d_stage_out.p : nullptr;
    BZH_TRY(scan_index_device(ctx, f, s, ctx->d_stage_in, n, idx, count, pts, npts, nullptr, found, out_total));
    return decode_unstage(ctx, out, out ? (size_t)*out_total : 0);
    });
}

// the public calls of the search: a byte string, or a set
extern "C" int bzh_search_raw_device(bzh_ctx *ctx, const void *d_raw, size_t n, const uint8_t *pat, size_t plen, unsigned flags, uint8_t delim,
                                     bzh_hit *hits, size_t max, size_t *nhits)
{
    SearchSink s(what_pat(pat, plen), flags, delim, hits, max);
    return scan_raw_device(ctx, SEARCH, s, d_raw, n, nhits, nullptr);
}
extern "C" int bzh_search_patset_raw_device(bzh_ctx *ctx, const void *d_raw, size_t n, const bzh_patset *set, unsigned flags, uint8_t delim,
                                            bzh_set_hit *hits, size_t max, size_t *nhits)
{
    SearchSink s(what_set(set), flags, delim, hits, max);
    return scan_raw_device(ctx, SEARCH, s, d_raw, n, nhits, nullptr);
}
extern "C" int bzh_search_device(bzh_ctx *ctx, const void *d_in, size_t n, const uint8_t *pat, size_t plen, unsigned flags, uint8_t delim,
                                 bzh_hit *hits, size_t max, size_t *nhits, uint64_t *out_total, size_t *consumed)
{
    SearchSink s(what_pat(pat, plen), flags, delim, hits, max);
    return scan_device(ctx, SEARCH, s, d_in, n, nhits, nullptr, out_total, consumed);
}
extern "C" int bzh_search_patset_device(bzh_ctx *ctx, const void *d_in, size_t n, const bzh_patset *set, unsigned flags, uint8_t delim,
                                        bzh_set_hit *hits, size_t max, size_t *nhits, uint64_t *out_total, size_t *consumed)
{
    SearchSink s(what_set(set), flags, delim, hits, max);
    return scan_device(ctx, SEARCH, s, d_in, n, nhits, nullptr, out_total, consumed);
}
extern "C" int bzh_search(bzh_ctx *ctx, const uint8_t *in, size_t n, const uint8_t *pat, size_t plen, unsigned flags, uint8_t delim,
                          bzh_hit *hits, size_t max, size_t *nhits, uint64_t *out_total, size_t *consumed)
{
    SearchSink s(what_pat(pat, plen), flags, delim, hits, max);
    return scan_host(ctx, SEARCH, s, in, n, nhits, nullptr, out_total, consumed);
}
extern "C" int bzh_search_patset(bzh_ctx *ctx, const uint8_t *in, size_t n, const bzh_patset *set, unsigned flags, uint8_t delim,
                                 bzh_set_hit *hits, size_t max, size_t *nhits, uint64_t *out_total, size_t *consumed)
{
    SearchSink s(what_set(set), flags, delim, hits, max);
    return scan_host(ctx, SEARCH, s, in, n, nhits, nullptr, out_total, consumed);
}
extern "C" int bzh_search_range_device(bzh_ctx *ctx, const void *d_in, size_t n, uint64_t in_byte_base, const bzh_index_entry *idx,
                                       size_t count, const bzh_sync_point *pts, size_t npts, const uint64_t *rec_cum, uint64_t off,
                                       uint64_t len, const uint8_t *pat, size_t plen, unsigned flags, uint8_t delim, bzh_hit *hits,
                                       size_t max, size_t *nhits)
{
    SearchSink s(what_pat(pat, plen), flags, delim, hits, max);
    const ScanRange range = {in_byte_base, rec_cum, off, len};
    return scan_index_device(ctx, SEARCH, s, d_in, n, idx, count, pts, npts, &range, nhits, nullptr);
}
extern "C" int bzh_search_patset_range_device(bzh_ctx *ctx, const void *d_in, size_t n, uint64_t in_byte_base, const bzh_index_entry *idx,
                                              size_t count, const bzh_sync_point *pts, size_t npts, const uint64_t *rec_cum, uint64_t off,
                                              uint64_t len, const bzh_patset *set, unsigned flags, uint8_t delim, bzh_set_hit *hits, size_t max,
                                              size_t *nhits)
{
    SearchSink s(what_set(set), flags, delim, hits, max);
    const ScanRange range = {in_byte_base, rec_cum, off, len};
    return scan_index_device(ctx, SEARCH, s, d_in, n, idx, count, pts, npts, &range, nhits, nullptr);
}
extern "C" int bzh_search_range(bzh_ctx *ctx, const uint8_t *in, size_t n, uint64_t in_byte_base, const bzh_index_entry *idx, size_t count,
                                const bzh_sync_point *pts, size_t npts, const uint64_t *rec_cum, uint64_t off, uint64_t len,
                                const uint8_t *pat, size_t plen, unsigned flags, uint8_t delim, bzh_hit *hits, size_t max, size_t *nhits)
{
    SearchSink s(what_pat(pat, plen), flags, delim, hits, max);
    const ScanRange range = {in_byte_base, rec_cum, off, len};
    return scan_index_host(ctx, SEARCH, s, in, n, idx, count, pts, npts, &range, nhits, nullptr);
}
extern "C" int bzh_search_patset_range(bzh_ctx *ctx, const uint8_t *in, size_t n, uint64_t in_byte_base, const bzh_index_entry *idx, size_t count,
                                       const bzh_sync_point *pts, size_t npts, const uint64_t *rec_cum, uint64_t off, uint64_t len,
                                       const bzh_patset *set, unsigned flags, uint8_t delim, bzh_set_hit *hits, size_t max, size_t *nhits)
{
    SearchSink s(what_set(set), flags, delim, hits, max);
    const ScanRange range = {in_byte_base, rec_cum, off, len};
    return scan_index_host(ctx, SEARCH, s, in, n, idx, count, pts, npts, &range, nhits, nullptr);
}

extern "C" int bzh_search_set_room(bzh_ctx *ctx, size_t bytes)
{
    return bzh_guard(ctx, [&]() -> int {
    if (!ctx) return BZH_E_ARG;
    if (bytes && bytes < 1024) {
        bzh_set_error(ctx, "search: a room of %zu bytes, below 1024", bytes);
        return BZH_E_ARG;
    }
    ctx->search_room = bytes;
    return BZH_OK;
    });
}

extern "C" int bzh_get_search_stats(const bzh_ctx *ctx, bzh_search_stats *out) { return stats_get(ctx, &bzh_ctx::sstats, out); }

// ... of the grep (its context setting is read when the sink is armed)
extern "C" int bzh_grep_raw_device(bzh_ctx *ctx, const void *d_raw, size_t n, const uint8_t *pat, size_t plen, unsigned flags, uint8_t delim,
                                   void *d_out, size_t cap, bzh_grep_entry *ent, size_t max, size_t *nrecs, uint64_t *out_total)
{
    GrepSink s(what_pat(pat, plen), flags, delim, d_out, cap, ent, max);
    return scan_raw_device(ctx, GREP, s, d_raw, n, nrecs, out_total);
}
extern "C" int bzh_grep_patset_raw_device(bzh_ctx *ctx, const void *d_raw, size_t n, const bzh_patset *set, unsigned flags, uint8_t delim,
                                          void *d_out, size_t cap, bzh_grep_entry *ent, size_t max, size_t *nrecs, uint64_t *out_total)
{
    GrepSink s(what_set(set), flags, delim, d_out, cap, ent, max);
    return scan_raw_device(ctx, GREP, s, d_raw, n, nrecs, out_total);
}
extern "C" int bzh_grep_device(bzh_ctx *ctx, const void *d_in, size_t n, const uint8_t *pat, size_t plen, unsigned flags, uint8_t delim,
                               void *d_out, size_t cap, bzh_grep_entry *ent, size_t max, size_t *nrecs, uint64_t *out_total,
                               uint64_t *decoded_total, size_t *consumed)
{
    GrepSink s(what_pat(pat, plen), flags, delim, d_out, cap, ent, max);
    return scan_device(ctx, GREP, s, d_in, n, nrecs, out_total, decoded_total, consumed);
}
extern "C" int bzh_grep_patset_device(bzh_ctx *ctx, const void *d_in, size_t n, const bzh_patset *set, unsigned flags, uint8_t delim,
                                      void *d_out, size_t cap, bzh_grep_entry *ent, size_t max, size_t *nrecs, uint64_t *out_total,
                                      uint64_t *decoded_total, size_t *consumed)
{
    GrepSink s(what_set(set), flags, delim, d_out, cap, ent, max);
    return scan_device(ctx, GREP, s, d_in, n, nrecs, out_total, decoded_total, consumed);
}
extern "C" int bzh_grep(bzh_ctx *ctx, const uint8_t *in, size_t n, const uint8_t *pat, size_t plen, unsigned flags, uint8_t delim,
                        uint8_t *out, size_t cap, bzh_grep_entry *ent, size_t max, size_t *nrecs, uint64_t *out_total,
                        uint64_t *decoded_total, size_t *consumed)
{
    GrepSink s(what_pat(pat, plen), flags, delim, out, cap, ent, max);
    return scan_host(ctx, GREP, s, in, n, nrecs, out_total, decoded_total, consumed);
}
extern "C" int bzh_grep_patset(bzh_ctx *ctx, const uint8_t *in, size_t n, const bzh_patset *set, unsigned flags, uint8_t delim, uint8_t *out,
                               size_t cap, bzh_grep_entry *ent, size_t max, size_t *nrecs, uint64_t *out_total, uint64_t *decoded_total,
                               size_t *consumed)
{
    GrepSink s(what_set(set), flags, delim, out, cap, ent, max);
    return scan_host(ctx, GREP, s, in, n, nrecs, out_total, decoded_total, consumed);
}
extern "C" int bzh_grep_index_device(bzh_ctx *ctx, const void *d_in, size_t n, const bzh_index_entry *idx, size_t count,
                                     const bzh_sync_point *pts, size_t npts, const uint8_t *pat, size_t plen, unsigned flags, uint8_t delim,
                                     void *d_out, size_t cap, bzh_grep_entry *ent, size_t max, size_t *nrecs, uint64_t *out_total)
{
    GrepSink s(what_pat(pat, plen), flags, delim, d_out, cap, ent, max);
    return scan_index_device(ctx, GREP, s, d_in, n, idx, count, pts, npts, nullptr, nrecs, out_total);
}
extern "C" int bzh_grep_patset_index_device(bzh_ctx *ctx, const void *d_in, size_t n, const bzh_index_entry *idx, size_t count,
                                            const bzh_sync_point *pts, size_t npts, const bzh_patset *set, unsigned flags, uint8_t delim,
                                            void *d_out, size_t cap, bzh_grep_entry *ent, size_t max, size_t *nrecs, uint64_t *out_total)
{
    GrepSink s(what_set(set), flags, delim, d_out, cap, ent, max);
    return scan_index_device(ctx, GREP, s, d_in, n, idx, count, pts, npts, nullptr, nrecs, out_total);
}
extern "C" int bzh_grep_index(bzh_ctx *ctx, const uint8_t *in, size_t n, const bzh_index_entry *idx, size_t count,
                              const bzh_sync_point *pts, size_t npts, const uint8_t *pat, size_t plen, unsigned flags, uint8_t delim,
                              uint8_t *out, size_t cap, bzh_grep_entry *ent, size_t max, size_t *nrecs, uint64_t *out_total)
{
    GrepSink s(what_pat(pat, plen), flags, delim, out, cap, ent, max);
    return scan_index_host(ctx, GREP, s, in, n, idx, count, pts, npts, nullptr, nrecs, out_total);
}
extern "C" int bzh_grep_patset_index(bzh_ctx *ctx, const uint8_t *in, size_t n, const bzh_index_entry *idx, size_t count,
                                     const bzh_sync_point *pts, size_t npts, const bzh_patset *set, unsigned flags, uint8_t delim, uint8_t *out,
                                     size_t cap, bzh_grep_entry *ent, size_t max, size_t *nrecs, uint64_t *out_total)
{
    GrepSink s(what_set(set), flags, delim, out, cap, ent, max);
    return scan_index_host(ctx, GREP, s, in, n, idx, count, pts, npts, nullptr, nrecs, out_total);
}

extern "C" int bzh_get_grep_stats(const bzh_ctx *ctx, bzh_grep_stats *out) { return stats_get(ctx, &bzh_ctx::gstats, out); }

extern "C" int bzh_grep_set_context(bzh_ctx *ctx, uint32_t before, uint32_t after)
{
    return bzh_guard(ctx, [&]() -> int {
    if (!ctx) return BZH_E_ARG;
    ctx->grep_before = before, ctx->grep_after = after;
    return BZH_OK;
    });
}

extern "C" int bzh_get_grep_context_stats(const bzh_ctx *ctx, bzh_grep_context_stats *out) { return stats_get(ctx, &bzh_ctx::gcstats, out); }

// ... of the matched parts alone
extern "C" int bzh_match_raw_device(bzh_ctx *ctx, const void *d_raw, size_t n, const uint8_t *pat, size_t plen, unsigned flags, uint8_t delim,
                                    void *d_out, size_t cap, bzh_match_entry *ent, size_t max, size_t *nmatches, uint64_t *out_total)
{
    MatchSink s(what_pat(pat, plen), flags, delim, d_out, cap, ent, max);
    return scan_raw_device(ctx, MATCH, s, d_raw, n, nmatches, out_total);
}
extern "C" int bzh_match_patset_raw_device(bzh_ctx *ctx, const void *d_raw, size_t n, const bzh_patset *set, unsigned flags, uint8_t delim,
                                           void *d_out, size_t cap, bzh_match_entry *ent, size_t max, size_t *nmatches, uint64_t *out_total)
{
    MatchSink s(what_set(set), flags, delim, d_out, cap, ent, max);
    return scan_raw_device(ctx, MATCH, s, d_raw, n, nmatches, out_total);
}
extern "C" int bzh_match_device(bzh_ctx *ctx, const void *d_in, size_t n, const uint8_t *pat, size_t plen, unsigned flags, uint8_t delim,
                                void *d_out, size_t cap, bzh_match_entry *ent, size_t max, size_t *nmatches, uint64_t *out_total,
                                uint64_t *decoded_total, size_t *consumed)
{
    MatchSink s(what_pat(pat, plen), flags, delim, d_out, cap, ent, max);
    return scan_device(ctx, MATCH, s, d_in, n, nmatches, out_total, decoded_total, consumed);
}
extern "C" int bzh_match_patset_device(bzh_ctx *ctx, const void *d_in, size_t n, const bzh_patset *set, unsigned flags, uint8_t delim,
                                       void *d_out, size_t cap, bzh_match_entry *ent, size_t max, size_t *nmatches, uint64_t *out_total,
                                       uint64_t *decoded_total, size_t *consumed)
{
    MatchSink s(what_set(set), flags, delim, d_out, cap, ent, max);
    return scan_device(ctx, MATCH, s, d_in, n, nmatches, out_total, decoded_total, consumed);
}
extern "C" int bzh_match(bzh_ctx *ctx, const uint8_t *in, size_t n, const uint8_t *pat, size_t plen, unsigned flags, uint8_t delim,
                         uint8_t *out, size_t cap, bzh_match_entry *ent, size_t max, size_t *nmatches, uint64_t *out_total,
                         uint64_t *decoded_total, size_t *consumed)
{
    MatchSink s(what_pat(pat, plen), flags, delim, out, cap, ent, max);
    return scan_host(ctx, MATCH, s, in, n, nmatches, out_total, decoded_total, consumed);
}
extern "C" int bzh_match_patset(bzh_ctx *ctx, const uint8_t *in, size_t n, const bzh_patset *set, unsigned flags, uint8_t delim, uint8_t *out,
                                size_t cap, bzh_match_entry *ent, size_t max, size_t *nmatches, uint64_t *out_total, uint64_t *decoded_total,
                                size_t *consumed)
{
    MatchSink s(what_set(set), flags, delim, out, cap, ent, max);
    return scan_host(ctx, MATCH, s, in, n, nmatches, out_total, decoded_total, consumed);
}
extern "C" int bzh_match_index_device(bzh_ctx *ctx, const void *d_in, size_t n, const bzh_index_entry *idx, size_t count,
                                      const bzh_sync_point *pts, size_t npts, const uint8_t *pat, size_t plen, unsigned flags, uint8_t delim,
                                      void *d_out, size_t cap, bzh_match_entry *ent, size_t max, size_t *nmatches, uint64_t *out_total)
{
    MatchSink s(what_pat(pat, plen), flags, delim, d_out, cap, ent, max);
    return scan_index_device(ctx, MATCH, s, d_in, n, idx, count, pts, npts, nullptr, nmatches, out_total);
}
extern "C" int bzh_match_patset_index_device(bzh_ctx *ctx, const void *d_in, size_t n, const bzh_index_entry *idx, size_t count,
                                             const bzh_sync_point *pts, size_t npts, const bzh_patset *set, unsigned flags, uint8_t delim,
                                             void *d_out, size_t cap, bzh_match_entry *ent, size_t max, size_t *nmatches, uint64_t *out_total)
{
    MatchSink s(what_set(set), flags, delim, d_out, cap, ent, max);
    return scan_index_device(ctx, MATCH, s, d_in, n, idx, count, pts, npts, nullptr, nmatches, out_total);
}
extern "C" int bzh_match_index(bzh_ctx *ctx, const uint8_t *in, size_t n, const bzh_index_entry *idx, size_t count,
                               const bzh_sync_point *pts, size_t npts, const uint8_t *pat, size_t plen, unsigned flags, uint8_t delim,
                               uint8_t *out, size_t cap, bzh_match_entry *ent, size_t max, size_t *nmatches, uint64_t *out_total)
{
    MatchSink s(what_pat(pat, plen), flags, delim, out, cap, ent, max);
    return scan_index_host(ctx, MATCH, s, in, n, idx, count, pts, npts, nullptr, nmatches, out_total);
}
extern "C" int bzh_match_patset_index(bzh_ctx *ctx, const uint8_t *in, size_t n, const bzh_index_entry *idx, size_t count,
                                      const bzh_sync_point *pts, size_t npts, const bzh_patset *set, unsigned flags, uint8_t delim, uint8_t *out,
                                      size_t cap, bzh_match_entry *ent, size_t max, size_t *nmatches, uint64_t *out_total)
{
    MatchSink s(what_set(set), flags, delim, out, cap, ent, max);
    return scan_index_host(ctx, MATCH, s, in, n, idx, count, pts, npts, nullptr, nmatches, out_total);
}

extern "C" int bzh_get_match_stats(const bzh_ctx *ctx, bzh_match_stats *out) { return stats_get(ctx, &bzh_ctx::mtstats, out); }

extern "C" int bzh_get_decode_ranges_stats(const bzh_ctx *ctx, bzh_decode_ranges_stats *out) { return stats_get(ctx, &bzh_ctx::qstats, out); }

extern "C" int bzh_get_decode_stats(const bzh_ctx *ctx, bzh_decode_stats *out) { return stats_get(ctx, &bzh_ctx::dstats, out); }

// ---- many inputs (decode.hip's decode_many_run): one scan of the whole buffer, the arena for a batch of its candidates
extern "C" int bzh_decode_many_device(bzh_ctx *ctx, const void *d_in, size_t n, const size_t *in_offs, const size_t *in_lens, size_t count,
                                      void *d_out, size_t cap, size_t *out_offs, size_t *out_lens, int *status, size_t *consumed)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || (!d_in && n) || (!d_out && cap)) return BZH_E_ARG;
    if (count && (!in_offs || !in_lens || !out_offs || !out_lens || !status)) {
        bzh_set_error(ctx, "decode many: a null array for %zu inputs", count);
        return BZH_E_ARG;
    }
    if (count > 0x7FFFFFFFull) {
        bzh_set_error(ctx, "decode many: %zu inputs are beyond one call", count);
        return BZH_E_ARG;
    }
    size_t end = 0; // of the slices so far
    for (size_t k = 0; k < count; k++) {
        if (in_offs[k] < end || in_offs[k] > n || in_lens[k] > n - in_offs[k]) {
            bzh_set_error(ctx, "decode many: input %zu is bytes [%zu, +%zu): %s", k, in_offs[k], in_lens[k],
                          in_offs[k] < end ? "the slices must ascend and must not overlap" : "past the end of the buffer");
            return BZH_E_ARG;
        }
        end = in_offs[k] + in_lens[k];
    }
    DecodeCall call;
    BZH_TRY(decode_call_begin(ctx, n, call));
    memset(&ctx->mstats, 0, sizeof ctx->mstats);
    if (count == 0) return decode_call_end(ctx, call, BZH_OK);
    std::vector<uint64_t> cands;
    BZH_TRY(decode_call_scan(ctx, call, d_in, n, cands));
    const int rc = decode_many_run(ctx, (const uint8_t *)d_in, n, in_offs, in_lens, count, (uint8_t *)d_out, cap, out_offs, out_lens, status,
                                   consumed, cands);
    return decode_call_end(ctx, call, rc);
    });
}

extern "C" int bzh_decode_many(bzh_ctx *ctx, const uint8_t *const *ins, const size_t *lens, size_t count, uint8_t *out, size_t cap,
                               size_t *out_offs, size_t *out_lens, int *status, size_t *consumed)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || (!out && cap)) return BZH_E_ARG;
    if (count && (!ins || !lens || !out_offs || !out_lens || !status)) {
        bzh_set_error(ctx, "decode many: a null array for %zu inputs", count);
        return BZH_E_ARG;
    }
    size_t total = 0;
    std::vector<size_t> offs(count);
    for (size_t k = 0; k < count; k++) {
        if (!ins[k] && lens[k]) {
            bzh_set_error(ctx, "decode many: input %zu is null with %zu bytes claimed", k, lens[k]);
            return BZH_E_ARG;
        }
        offs[k] = total;
        total += lens[k];
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    BZH_TRY(ensure_stage(ctx, ctx->d_stage_in, total + 16));
    if (cap) BZH_TRY(ensure_stage(ctx, ctx->d_stage_out, cap));
    if (total) { // all inputs in one copy, back to back
        ctx->many_pack.resize(total);
        for (size_t k = 0; k < count; k++)
            if (lens[k]) memcpy(ctx->many_pack.data() + offs[k], ins[k], lens[k]);
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_stage_in, ctx->many_pack.data(), total, hipMemcpyHostToDevice, ctx->stream));
    }
    BZH_TRY(bzh_decode_many_device(ctx, ctx->d_stage_in, total, offs.data(), lens, count, cap ? ctx->d_stage_out : nullptr, cap, out_offs,
                                   out_lens, status, consumed));
    const size_t len = count ? out_offs[count - 1] + out_lens[count - 1] : 0;
    if (len) HIP_TRY(ctx, hipMemcpyAsync(out, ctx->d_stage_out, len, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, bzh_stream_wait(ctx->stream));
    return BZH_OK;
    });
}

extern "C" int bzh_get_decode_many_stats(const bzh_ctx *ctx, bzh_decode_many_stats *out) { return stats_get(ctx, &bzh_ctx::mstats, out); }

// ---- grep over many inputs (grep_many.hip's GrepSink::raw_many; the tables: grep_many_plan.h).  Three routes to the one segmented
// pass: texts that lie in HBM, inputs decoded by bzh_decode_many_device into the grep's staging buffer, and the latter from the host.
static_assert(sizeof(bzh_grep_many_item) == 40, "an item is five words");

// what every route checks first, in scan_begin's order; behind it the statistics are fresh and the sink is armed
static int grep_many_begin(bzh_ctx *ctx, GrepSink &s, size_t count, const void *a0, const void *a1, bzh_grep_many_item *items, size_t *nrecs,
                           uint64_t *out_total)
{
    if (count && (!a0 || !a1 || !items)) {
        bzh_set_error(ctx, "grep many: a null array for %zu inputs", count);
        return BZH_E_ARG;
    }
    BZH_TRY(scan_begin(ctx, GREP, s, nrecs, out_total));
    memset(&ctx->gmstats, 0, sizeof ctx->gmstats);
    if (count) memset(items, 0, count * sizeof *items);
    if (s.ctx_on) {
        bzh_set_error(ctx, "grep many: context records are set (bzh_grep_set_context %u, %u) and are not built over many inputs; set 0, 0",
                      ctx->grep_before, ctx->grep_after);
        return BZH_E_ARG;
    }
    if (count > 0x7FFFFFFFull) {
        bzh_set_error(ctx, "grep many: %zu inputs are beyond one call", count);
        return BZH_E_ARG;
    }
    return BZH_OK;
}

// The pass over checked segments of d_raw, what the sink held back (nothing), the last wait, and the answer.  status: of every
// input (null: all BZH_OK); a failed one has an empty segment.
static int grep_many_pass(bzh_ctx *ctx, GrepSink &s, const uint8_t *d_raw, const uint64_t *offs, const uint64_t *lens, const int *status, size_t count,
                          bzh_grep_many_item *items, size_t *nrecs, uint64_t *out_total)
{
    BzgmPlan plan;
    bzh_grep_many_stats &gm = ctx->gmstats;
    const bool built = plan.build(offs, lens, count);
    gm.inputs = count, gm.segments = plan.nonempty, gm.virtual_tiles = plan.rows, gm.shared_tiles = plan.shared;
    if (!built) {
        bzh_set_error(ctx, "grep many: %llu virtual tiles are beyond one launch", (unsigned long long)plan.rows);
        return BZH_E_ARG;
    }
    std::vector<uint64_t> tot(count * BZGM_TOTALS);
    int rc = s.raw_many(ctx, d_raw, plan, tot.data());
    if (rc == BZH_OK) rc = s.finish(ctx);
    HIP_TRY(ctx, bzh_stream_wait(ctx->stream));
    if (rc != BZH_OK) return rc;
    for (size_t k = 0; k < count; k++) {
        const uint64_t *t = &tot[k * BZGM_TOTALS];
        items[k] = bzh_grep_many_item{lens[k], t[BZGM_T_RECORDS], t[BZGM_T_SEL], t[BZGM_T_BYTES], status ? status[k] : BZH_OK, 0};
        if (items[k].status != BZH_OK) gm.inputs_failed++;
    }
    return s.report(ctx, nrecs, out_total);
}

static int grep_many_raw_device(bzh_ctx *ctx, GrepSink &s, const void *d_raw, size_t n, const size_t *offs, const size_t *lens, size_t count,
                                bzh_grep_many_item *items, size_t *nrecs, uint64_t *out_total)
{
    return bzh_guard(ctx, [&]() -> int {
    static_assert(sizeof(size_t) == 8, "the segments are 64-bit words");
    if (ctx) stream_join(ctx);
    if (!ctx || (!d_raw && n)) return BZH_E_ARG;
    BZH_TRY(grep_many_begin(ctx, s, count, offs, lens, items, nrecs, out_total));
    if ((uintptr_t)d_raw & 15u) {
        bzh_set_error(ctx, "grep many: the buffer is not 16-byte aligned");
        return BZH_E_ARG;
    }
    size_t bad = 0;
    if (const char *what = bzgm_check((const uint64_t *)offs, (const uint64_t *)lens, count, n, &bad)) {
        bzh_set_error(ctx, "grep many: segment %zu is bytes [%zu, +%zu): %s", bad, offs[bad], lens[bad], what);
        return BZH_E_ARG;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return grep_many_pass(ctx, s, (const uint8_t *)d_raw, (const uint64_t *)offs, (const uint64_t *)lens, nullptr, count, items, nrecs, out_total);
    });
}

// the first size of the staging buffer, from the compressed bytes: text rarely expands beyond six times
static size_t grep_many_stage_guess(size_t n) { return n > (~(size_t)0 >> 4) ? n : 6 * n + ((size_t)1 << 20); }

static int grep_many_device(bzh_ctx *ctx, GrepSink &s, const void *d_in, size_t n, const size_t *in_offs, const size_t *in_lens, size_t count,
                            bzh_grep_many_item *items, size_t *nrecs, uint64_t *out_total)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || (!d_in && n)) return BZH_E_ARG;
    BZH_TRY(grep_many_begin(ctx, s, count, in_offs, in_lens, items, nrecs, out_total));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<size_t> out_offs(count), out_lens(count);
    std::vector<int> status(count);
    size_t room = grep_many_stage_guess(n);
    uint64_t retries = 0;
    for (;;) { // (at most twice: the second room is the one the walk asked for)
        BZH_TRY(ctx->search_ws.reserve(ctx, room + 16, "the grep's staging", grow_mib));
        ctx->gstats.staging_peak = ctx->search_ws.cap;
        const int rc = bzh_decode_many_device(ctx, d_in, n, in_offs, in_lens, count, ctx->search_ws.p, room, out_offs.data(), out_lens.data(),
                                              status.data(), nullptr);
        if (rc == BZH_E_CAP && !retries && count) {
            // the walk's total, the gaps that failed inputs leave included: a failed input has out_lens 0, so the last offset
            // and length alone fall short where trailing inputs failed behind placed blocks
            room = std::max<size_t>((size_t)ctx->dstats.out_bytes, out_offs[count - 1] + out_lens[count - 1]);
            retries++;
            continue;
        }
        BZH_TRY(rc);
        break;
    }
    // a failed input owns no byte: an empty segment where the one in front of it ends
    std::vector<uint64_t> offs(count), lens(count);
    uint64_t end = 0;
    for (size_t k = 0; k < count; k++) {
        const bool ok = status[k] == BZH_OK;
        offs[k] = ok ? out_offs[k] : end, lens[k] = ok ? out_lens[k] : 0;
        end = offs[k] + lens[k];
    }
    const uint64_t staging = ctx->gstats.staging_peak;
    const int rc = grep_many_pass(ctx, s, ctx->search_ws.p, offs.data(), lens.data(), status.data(), count, items, nrecs, out_total);
    ctx->gstats.staging_peak = staging; // (finish() leaves the other counters of the pass)
    ctx->gmstats.staging_retries = retries;
    return rc;
    });
}

static int grep_many_host(bzh_ctx *ctx, GrepSink &s, const uint8_t *const *ins, const size_t *lens, size_t count, bzh_grep_many_item *items,
                          size_t *nrecs, uint64_t *out_total)
{
    return bzh_guard(ctx, [&]() -> int {
    uint8_t *const out = (uint8_t *)s.args.out;
    if (ctx) stream_join(ctx);
    if (!ctx || (!out && s.args.cap)) return BZH_E_ARG;
    // (as scan_host: the device route begins the call, with the staged output in the caller's place -- a host buffer needs no
    // alignment; here only what the packing itself reads)
    if (count && (!ins || !lens || !items)) {
        bzh_set_error(ctx, "grep many: a null array for %zu inputs", count);
        return BZH_E_ARG;
    }
    if (!nrecs || !out_total) return BZH_E_ARG;
    *nrecs = 0, *out_total = 0;
    size_t total = 0;
    std::vector<size_t> offs(count);
    for (size_t k = 0; k < count; k++) {
        if (!ins[k] && lens[k]) {
            bzh_set_error(ctx, "grep many: input %zu is null with %zu bytes claimed", k, lens[k]);
            return BZH_E_ARG;
        }
        offs[k] = total;
        total += lens[k];
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    BZH_TRY(ensure_stage(ctx, ctx->d_stage_in, total + 16));
    if (out) BZH_TRY(ensure_stage(ctx, ctx->d_stage_out, scan_stage_room(out, s.args.cap)));
    if (total) { // all inputs in one copy, back to back
        ctx->many_pack.resize(total);
        for (size_t k = 0; k < count; k++)
            if (lens[k]) memcpy(ctx->many_pack.data() + offs[k], ins[k], lens[k]);
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_stage_in, ctx->many_pack.data(), total, hipMemcpyHostToDevice, ctx->stream));
    }
    s.args.out = out ? ctx->d_stage_out.p : nullptr;
    BZH_TRY(grep_many_device(ctx, s, ctx->d_stage_in, total, offs.data(), lens, count, items, nrecs, out_total));
    return decode_unstage(ctx, out, out ? (size_t)*out_total : 0);
    });
}

extern "C" int bzh_grep_many_raw_device(bzh_ctx *ctx, const void *d_raw, size_t n, const size_t *offs, const size_t *lens, size_t count,
                                        const uint8_t *pat, size_t plen, unsigned flags, uint8_t delim, void *d_out, size_t cap,
                                        bzh_grep_entry *ent, size_t max, bzh_grep_many_item *items, size_t *nrecs, uint64_t *out_total)
{
    GrepSink s(what_pat(pat, plen), flags, delim, d_out, cap, ent, max);
    return grep_many_raw_device(ctx, s, d_raw, n, offs, lens, count, items, nrecs, out_total);
}
extern "C" int bzh_grep_many_patset_raw_device(bzh_ctx *ctx, const void *d_raw, size_t n, const size_t *offs, const size_t *lens, size_t count,
                                               const bzh_patset *set, unsigned flags, uint8_t delim, void *d_out, size_t cap,
                                               bzh_grep_entry *ent, size_t max, bzh_grep_many_item *items, size_t *nrecs, uint64_t *out_total)
{
    GrepSink s(what_set(set), flags, delim, d_out, cap, ent, max);
    return grep_many_raw_device(ctx, s, d_raw, n, offs, lens, count, items, nrecs, out_total);
}
extern "C" int bzh_grep_many_device(bzh_ctx *ctx, const void *d_in, size_t n, const size_t *in_offs, const size_t *in_lens, size_t count,
                                    const uint8_t *pat, size_t plen, unsigned flags, uint8_t delim, void *d_out, size_t cap,
                                    bzh_grep_entry *ent, size_t max, bzh_grep_many_item *items, size_t *nrecs, uint64_t *out_total)
{
    GrepSink s(what_pat(pat, plen), flags, delim, d_out, cap, ent, max);
    return grep_many_device(ctx, s, d_in, n, in_offs, in_lens, count, items, nrecs, out_total);
}
extern "C" int bzh_grep_many_patset_device(bzh_ctx *ctx, const void *d_in, size_t n, const size_t *in_offs, const size_t *in_lens, size_t count,
                                           const bzh_patset *set, unsigned flags, uint8_t delim, void *d_out, size_t cap,
                                           bzh_grep_entry *ent, size_t max, bzh_grep_many_item *items, size_t *nrecs, uint64_t *out_total)
{
    GrepSink s(what_set(set), flags, delim, d_out, cap, ent, max);
    return grep_many_device(ctx, s, d_in, n, in_offs, in_lens, count, items, nrecs, out_total);
}
extern "C" int bzh_grep_many(bzh_ctx *ctx, const uint8_t *const *ins, const size_t *lens, size_t count, const uint8_t *pat, size_t plen,
                             unsigned flags, uint8_t delim, uint8_t *out, size_t cap, bzh_grep_entry *ent, size_t max,
                             bzh_grep_many_item *items, size_t *nrecs, uint64_t *out_total)
{
    GrepSink s(what_pat(pat, plen), flags, delim, out, cap, ent, max);
    return grep_many_host(ctx, s, ins, lens, count, items, nrecs, out_total);
}
extern "C" int bzh_grep_many_patset(bzh_ctx *ctx, const uint8_t *const *ins, const size_t *lens, size_t count, const bzh_patset *set,
                                    unsigned flags, uint8_t delim, uint8_t *out, size_t cap, bzh_grep_entry *ent, size_t max,
                                    bzh_grep_many_item *items, size_t *nrecs, uint64_t *out_total)
{
    GrepSink s(what_set(set), flags, delim, out, cap, ent, max);
    return grep_many_host(ctx, s, ins, lens, count, items, nrecs, out_total);
}

extern "C" int bzh_get_grep_many_stats(const bzh_ctx *ctx, bzh_grep_many_stats *out) { return stats_get(ctx, &bzh_ctx::gmstats, out); }

// ---- recovery (decode.hip's decode_recover_run; recover.hip's gather): per block what bzh_decode is per input
extern "C" int bzh_recover_device(bzh_ctx *ctx, const void *d_in, size_t n, void *d_out, size_t cap, size_t *out_len, bzh_recover_entry *ent,
                                  size_t max, size_t *count)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || (!d_in && n) || (!d_out && cap) || !out_len || (!ent && max) || !count) return BZH_E_ARG;
    DecodeCall call;
    BZH_TRY(decode_call_begin(ctx, n, call));
    memset(&ctx->rstats, 0, sizeof ctx->rstats);
    *out_len = 0;
    *count = 0;
    std::vector<uint64_t> cands;
    BZH_TRY(decode_call_scan(ctx, call, d_in, n, cands));
    std::vector<bzh_recover_entry> entries;
    int rc = decode_recover_run(ctx, (const uint8_t *)d_in, n, (uint8_t *)d_out, cap, out_len, entries, ctx->rstats, cands);
    rc = decode_call_end(ctx, call, rc);
    if (rc != BZH_OK && rc != BZH_E_CAP) return rc;
    bzh_decode_stats &ds = ctx->dstats;
    ds.blocks = ctx->rstats.kept;
    ds.streams = ctx->rstats.streams_ok;
    ds.candidates_off_chain = ctx->rstats.shadowed;
    ds.out_bytes = ctx->rstats.out_bytes;
    *count = entries.size();
    if (entries.size() > max) {
        bzh_set_error(ctx, "recover: %zu entries, room for %zu", entries.size(), max);
        return BZH_E_CAP;
    }
    if (!entries.empty()) memcpy(ent, entries.data(), entries.size() * sizeof(bzh_recover_entry));
    return rc;
    });
}

extern "C" int bzh_recover(bzh_ctx *ctx, const uint8_t *in, size_t n, uint8_t *out, size_t cap, size_t *out_len, bzh_recover_entry *ent,
                           size_t max, size_t *count)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || (!in && n) || (!out && cap) || !out_len || (!ent && max) || !count) return BZH_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    BZH_TRY(decode_stage(ctx, in, n, cap));
    size_t len = 0;
    const int rc = bzh_recover_device(ctx, ctx->d_stage_in, n, cap ? ctx->d_stage_out : nullptr, cap, &len, ent, max, count);
    *out_len = len; // (BZH_E_CAP: the size needed)
    if (len > cap || (rc != BZH_OK && rc != BZH_E_CAP)) return rc;
    if (len) HIP_TRY(ctx, hipMemcpyAsync(out, ctx->d_stage_out, len, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, bzh_stream_wait(ctx->stream));
    return rc;
    });
}

extern "C" int bzh_get_recover_stats(const bzh_ctx *ctx, bzh_recover_stats *out) { return stats_get(ctx, &bzh_ctx::rstats, out); }

// The report is checked as a whole and the size set before anything is launched; then the magics, the gather and the frame.
extern "C" int bzh_recover_stream_device(bzh_ctx *ctx, const void *d_in, size_t n, const bzh_recover_entry *ent, size_t count, void *d_out,
                                         size_t cap, size_t *out_len)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || (!d_in && n) || (!d_out && cap) || (!ent && count) || !out_len) return BZH_E_ARG;
    *out_len = 0;
    size_t bad = 0, kept = 0;
    uint64_t body = 0;
    if (const char *what = bzr_report_check(ent, count, n, &bad, &body, &kept)) {
        bzh_set_error(ctx, "recover stream: entry %zu: %s", bad, what);
        return BZH_E_ARG;
    }
    if (kept > 0x7FFFFFFFull) {
        bzh_set_error(ctx, "recover stream: %zu kept blocks are beyond one launch", kept);
        return BZH_E_ARG;
    }
    const uint64_t total_bits = 32 + body + 80;
    const size_t bytes = (size_t)((total_bits + 7) / 8), words = (size_t)((total_bits + 31) / 32);
    *out_len = bytes;
    if (words * 4 > cap) {
        bzh_set_error(ctx, "recover stream: the stream needs %zu bytes (%zu as whole words), the buffer holds %zu", bytes, words * 4, cap);
        return BZH_E_CAP;
    }
    if (((uintptr_t)d_out & 3u) != 0) {
        bzh_set_error(ctx, "recover stream: the output is not 4-byte aligned");
        return BZH_E_ARG;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    std::vector<BzrDesc> descs;
    std::vector<uint64_t> pos;
    std::vector<size_t> entry_of;
    std::vector<uint32_t> crcs;
    descs.reserve(kept), pos.reserve(kept), entry_of.reserve(kept), crcs.reserve(kept);
    uint64_t at = 32;
    for (size_t k = 0; k < count; k++) {
        if (ent[k].kind != 0) continue;
        descs.push_back(BzrDesc{ent[k].bit_pos, at, ent[k].end_bit - ent[k].bit_pos});
        at += ent[k].end_bit - ent[k].bit_pos;
        pos.push_back(ent[k].bit_pos);
        entry_of.push_back(k);
        crcs.push_back(ent[k].crc);
    }
    size_t first_bad = kept;
    BZH_TRY(decode_magic_run(ctx, (const uint8_t *)d_in, n, pos.data(), kept, &first_bad));
    if (first_bad < kept) {
        bzh_set_error(ctx, "recover stream: entry %zu: no block magic at bit %llu", entry_of[first_bad], (unsigned long long)pos[first_bad]);
        return BZH_E_DATA;
    }
    // the gather writes the body's words whole; the header's word and the words the footer touches are ORed into
    const size_t wtail = (size_t)((32 + body) / 32);
    HIP_TRY(ctx, hipMemsetAsync(d_out, 0, 4, st));
    HIP_TRY(ctx, hipMemsetAsync((uint8_t *)d_out + wtail * 4, 0, (words - wtail) * 4, st));
    BZH_TRY(recover_gather_run(ctx, (const uint8_t *)d_in, n, descs, body, (uint32_t *)d_out));
    stream_frame<<<1, 64, 0, st>>>((uint32_t *)d_out, ctx->level, body, fold_stream_crc(crcs.data(), crcs.size()));
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, bzh_stream_wait(st));
    return BZH_OK;
    });
}

extern "C" int bzh_recover_stream(bzh_ctx *ctx, const uint8_t *in, size_t n, const bzh_recover_entry *ent, size_t count, uint8_t *out, size_t cap,
                                  size_t *out_len)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || (!in && n) || (!out && cap) || (!ent && count) || !out_len) return BZH_E_ARG;
    *out_len = 0;
    size_t bad = 0, kept = 0;
    uint64_t body = 0;
    if (const char *what = bzr_report_check(ent, count, n, &bad, &body, &kept)) {
        bzh_set_error(ctx, "recover stream: entry %zu: %s", bad, what);
        return BZH_E_ARG;
    }
    const size_t bytes = (size_t)((32 + body + 80 + 7) / 8), room = (bytes + 3) / 4 * 4;
    *out_len = bytes;
    if (bytes > cap) {
        bzh_set_error(ctx, "recover stream: the stream needs %zu bytes, the buffer holds %zu", bytes, cap);
        return BZH_E_CAP;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    BZH_TRY(decode_stage(ctx, in, n, room));
    size_t len = 0;
    BZH_TRY(bzh_recover_stream_device(ctx, ctx->d_stage_in, n, ent, count, ctx->d_stage_out, room, &len));
    HIP_TRY(ctx, hipMemcpyAsync(out, ctx->d_stage_out, len, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, bzh_stream_wait(ctx->stream));
    *out_len = len;
    return BZH_OK;
    });
}

extern "C" int bzh_decode_scan(bzh_ctx *ctx, const uint8_t *in, size_t n, uint64_t *bitpos, uint8_t *kind, size_t max, size_t *count)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || (!in && n) || !count || (max && (!bitpos || !kind))) return BZH_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    BZH_TRY(decode_stage(ctx, in, n));
    std::vector<uint64_t> cands;
    BZH_TRY(decode_scan_run(ctx, ctx->d_stage_in, n, cands));
    *count = cands.size();
    if (cands.size() > max) return BZH_E_CAP;
    for (size_t k = 0; k < cands.size(); k++) {
        bitpos[k] = cands[k] >> 1;
        kind[k] = (uint8_t)(cands[k] & 1u);
    }
    return BZH_OK;
    });
}


// ================================================================================================
// Many inputs, one stream each (bzh_encode_many*): N calls of banzai::encode (lib/lib.rs:84-132) in one pass -- one plan over
// all inputs (rle1_plan_many), then batches of blocks of any inputs, laid out, packed and framed on the device
// (huff_many_batch); the host waits for the plan and, at the end, for the offsets and lengths.  One lane (bzh_set_lanes does
// not apply).
// ================================================================================================
static size_t many_stream_bound(size_t len, size_t M)
{
    if (len == 0) return 14 + 3; // "BZh"+level, footer magic, CRC 0; alignment
    const size_t blocks = len / ((M - 1) * 4 / 5) + 1;
    const size_t rle = len + len / 4 + blocks * 8; // RLE1 grows by at most 5/4 (+ a run restarted at every cut)
    // at most one symbol per RLE1 byte + EOB, <= 17 bits each + 6 selector bits per 50 (2.2 bytes cover it), header and tables
    // of a block < 4,400 bytes (the comment above worst_case_slab, multi.hip), frame, alignment
    return rle * 22 / 10 + blocks * 4400 + 14 + 3;
}

extern "C" size_t bzh_encode_many_bound(int level, const size_t *lens, size_t count)
{
    if (level < 1 || level > 9 || (count && !lens)) return 0;
    const size_t M = 100000u * (size_t)level - 1u;
    size_t sum = 0;
    for (size_t k = 0; k < count; k++) sum += many_stream_bound(lens[k], M);
    return sum;
}

// The inputs' bytes must fit the plan's 32-bit positions together with one guard byte an input (rle1_plan_many).
static int many_range(bzh_ctx *ctx, const size_t *lens, size_t count, size_t *total)
{
    if (count && !lens) {
        bzh_set_error(ctx, "lens is null");
        return BZH_E_ARG;
    }
    const uint64_t lim = 0xFFFF0000ull;
    uint64_t tot = count;
    for (size_t k = 0; k < count; k++) {
        if (lens[k] > lim || tot + lens[k] > lim) {
            bzh_set_error(ctx, "%zu inputs exceed the 32-bit position range of one plan (bytes + one per input <= %llu)", count,
                          (unsigned long long)lim);
            return BZH_E_ARG;
        }
        tot += lens[k];
    }
    *total = (size_t)(tot - count);
    return BZH_OK;
}

static int many_in_args(bzh_ctx *ctx, const void *d_in, const size_t *lens, size_t count, size_t *total)
{
    BZH_TRY(many_range(ctx, lens, count, total));
    if (*total && !d_in) {
        bzh_set_error(ctx, "device input is null");
        return BZH_E_ARG;
    }
    return check_in_ptr(ctx, d_in);
}

extern "C" int bzh_plan_many_device(bzh_ctx *ctx, const void *d_in, const size_t *lens, size_t count, size_t *nblocks)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx || !nblocks) return BZH_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    size_t total = 0;
    BZH_TRY(many_in_args(ctx, d_in, lens, count, &total));
    BZH_TRY(rle1_plan_many(ctx, (const uint8_t *)d_in, lens, count));
    *nblocks = ctx->plan_blocks.size();
    return BZH_OK;
    });
}

static int encode_many(bzh_ctx *ctx, const void *d_in, const size_t *lens, size_t count, void *d_out, size_t cap, size_t *out_offs,
                       size_t *out_lens)
{
    size_t total = 0;
    BZH_TRY(many_in_args(ctx, d_in, lens, count, &total));
    if (count && (!d_out || !out_offs || !out_lens)) {
        bzh_set_error(ctx, "output pointers are null");
        return BZH_E_ARG;
    }
    if (((uintptr_t)d_out & 3u) != 0) {
        bzh_set_error(ctx, "output buffer must be 4-byte aligned");
        return BZH_E_ARG;
    }
    hipStream_t st = ctx->stream;
    stats_begin(ctx);
    if (count == 0) return BZH_OK;
    hipEvent_t t0 = call_mark(ctx);
    BZH_TRY(rle1_plan_many(ctx, (const uint8_t *)d_in, lens, count));
    hipEvent_t t1 = call_mark(ctx);
    // state | offs | lens | body | crc
    const size_t words = MST_WORDS + 3 * count + (count + 1) / 2;
    BZH_TRY(ctx->many_out.reserve(ctx, words * 8, "the layout of the streams"));
    ManyOut mo;
    mo.state = ctx->many_out.as<uint64_t>();
    mo.offs = mo.state + MST_WORDS;
    mo.lens = mo.offs + count;
    mo.body = mo.lens + count;
    mo.crc = reinterpret_cast<uint32_t *>(mo.body + count);
    HIP_TRY(ctx, hipMemsetAsync(ctx->many_out, 0, words * 8, st));
    const size_t nb = ctx->plan_blocks.size();
    const uint32_t per = ctx->max_batch;
    BZH_TRY(ensure_arena(ctx, (uint32_t)std::min<size_t>(std::max<size_t>(nb, 1), per)));
    ManyBatch mb{};
    mb.level = (uint32_t)ctx->level;
    mb.cap_words = cap / 4;
    std::vector<RangeJob> jobs;
    build_jobs(ctx, 0, nb, per, jobs);
    auto place = [&](size_t k0, uint32_t B, uint32_t mmax) -> int { // the streams of a batch (encode_plan.h), laid out and framed on the device
        const BzeMany d = bze_many_batch(ctx->plan_input.data(), k0, B, nb, count, mb.close_hi); // (close_hi: first input not complete)
        mb.B = B;
        mb.lo = d.lo;
        mb.lo_started = d.lo_started;
        mb.close_hi = d.close_hi;
        mb.hi = d.hi;
        return huff_many_batch(ctx, mb, B ? ctx->many_binp + k0 : nullptr, (uint8_t *)d_out, mmax, mo);
    };
    int status = nb ? BZH_OK : place(0, 0, 0); // (every input is empty: no batch, only frames)
    for (RangeJob &j : jobs) {
        if ((status = prepare_batch(ctx, j, false)) != BZH_OK || (status = place(j.k0, j.B, j.mmax)) != BZH_OK) break;
        j.ev[5] = call_mark(ctx);
    }
    if (status != BZH_OK) {
        (void)bzh_stream_wait(st); // (nothing of this call may still run when the error is reported)
        return status;
    }
    ctx->many_host.resize(MST_WORDS + 2 * count);
    HIP_TRY(ctx, hipMemcpyAsync(ctx->many_host.data(), mo.state, ctx->many_host.size() * 8, hipMemcpyDeviceToHost, st));
    hipEvent_t t2 = call_mark(ctx);
    HIP_TRY(ctx, bzh_stream_wait(st));
    const uint64_t *hs = ctx->many_host.data();
    if (hs[MST_OVER]) {
        bzh_set_error(ctx, "output needs %llu bytes, more than the %zu given", (unsigned long long)hs[MST_OFF], cap);
        return BZH_E_CAP;
    }
    for (size_t k = 0; k < count; k++) {
        out_offs[k] = (size_t)hs[MST_WORDS + k];
        out_lens[k] = (size_t)hs[MST_WORDS + count + k];
    }
    ctx->stats.out_bits = hs[MST_BITS];
    if (ctx->profiling) {
        jobs_ms(ctx, jobs);
        stats_collect_sort(ctx);
        ctx->stats.ms_plan = span_ms(t0, t1);
        ctx->stats.ms_total = span_ms(t0, t2);
    }
    return BZH_OK;
}

extern "C" int bzh_encode_many_device(bzh_ctx *ctx, const void *d_in, const size_t *lens, size_t count, void *d_out, size_t cap,
                                      size_t *out_offs, size_t *out_lens)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx) return BZH_E_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return encode_many(ctx, d_in, lens, count, d_out, cap, out_offs, out_lens);
    });
}

extern "C" int bzh_encode_many(bzh_ctx *ctx, const uint8_t *const *ins, const size_t *lens, size_t count, uint8_t *out, size_t cap,
                               size_t *out_offs, size_t *out_lens)
{
    return bzh_guard(ctx, [&]() -> int {
    if (ctx) stream_join(ctx);
    if (!ctx) return BZH_E_ARG;
    size_t total = 0;
    BZH_TRY(many_range(ctx, lens, count, &total));
    if (count && (!ins || !out || !out_offs || !out_lens)) {
        bzh_set_error(ctx, "null pointer among ins, out, out_offs, out_lens");
        return BZH_E_ARG;
    }
    for (size_t k = 0; k < count; k++)
        if (lens[k] && !ins[k]) {
            bzh_set_error(ctx, "input %zu is null", k);
            return BZH_E_ARG;
        }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    BZH_TRY(ensure_stage(ctx, ctx->d_stage_in, total + 16));
    BZH_TRY(ensure_stage(ctx, ctx->d_stage_out, bzh_encode_many_bound(ctx->level, lens, count) + 16));
    if (total) { // all inputs in one copy
        ctx->many_pack.resize(total);
        size_t pos = 0;
        for (size_t k = 0; k < count; k++) {
            if (lens[k]) memcpy(ctx->many_pack.data() + pos, ins[k], lens[k]);
            pos += lens[k];
        }
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_stage_in, ctx->many_pack.data(), total, hipMemcpyHostToDevice, st));
    }
    BZH_TRY(encode_many(ctx, ctx->d_stage_in, lens, count, ctx->d_stage_out, ctx->d_stage_out.cap & ~(size_t)3, out_offs, out_lens));
    const size_t need = count ? out_offs[count - 1] + out_lens[count - 1] : 0;
    if (need > cap) {
        bzh_set_error(ctx, "output needs %zu bytes, more than the %zu given", need, cap);
        return BZH_E_CAP;
    }
    if (need) {
        HIP_TRY(ctx, hipMemcpyAsync(out, ctx->d_stage_out, need, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, bzh_stream_wait(st));
    }
    return BZH_OK;
    });
}

// ================================================================================================
// Streaming
// ================================================================================================

static inline void put_be32(uint8_t *p, uint32_t v)
{
    p[0] = (uint8_t)(v >> 24);
    p[1] = (uint8_t)(v >> 16);
    p[2] = (uint8_t)(v >> 8);
    p[3] = (uint8_t)v;
}

// Waits for the pass in flight (if any); its results stay in strm.pass until stream_collect.
static void stream_join(bzh_ctx *ctx)
{
    auto &s = ctx->strm;
    if (s.worker.joinable()) s.worker.join();
}

// bzh_stream_begin, bzh_stream_begin_index (`index`: the stream records its index, with sync points every `interval` groups)
static int stream_begin(bzh_ctx *ctx, bool index, uint32_t interval)
{
    return bzh_guard(ctx, [&]() -> int {
    if (!ctx) return BZH_E_ARG;
    if (interval > 32767) {
        bzh_set_error(ctx, "stream index: a sync interval of %u groups, outside 0..32767", interval);
        return BZH_E_ARG;
    }
    auto &s = ctx->strm;
    stream_join(ctx);
    s.inflight = false;
    s.active = true;
    s.header_done = false;
    s.pending = 0;
    s.fill = 0;
    s.head = 0;
    s.bitpos = 0;
    s.carry_word = 0;
    s.stream_crc = 0;
    s.consumed = 0;
    s.index = index;
    s.interval = interval;
    s.ix_entries.clear();
    s.ix_pts.clear();
    s.ix_blocks = 0;
    return BZH_OK;
    });
}

extern "C" int bzh_stream_begin(bzh_ctx *ctx) { return stream_begin(ctx, false, 0); }

// ---- the streaming encoder records its index (stream_index.h) --------------------------------------------------------------
extern "C" int bzh_stream_begin_index(bzh_ctx *ctx, uint32_t interval) { return stream_begin(ctx, true, interval); }

// (No join: the fields read here belong to the feeding thread; the pass in flight fills strm.pass alone.)
extern "C" int bzh_stream_index_pending(const bzh_ctx *ctx, size_t *count, size_t *npts)
{
    if (!ctx) return BZH_E_ARG;
    if (count) *count = ctx->strm.ix_entries.size();
    if (npts) *npts = ctx->strm.ix_pts.size();
    return BZH_OK;
}

extern "C" int bzh_stream_index_take(bzh_ctx *ctx, bzh_index_entry *idx, size_t max, size_t *count, bzh_sync_point *pts, size_t max_pts,
                                     size_t *npts)
{
    return bzh_guard(ctx, [&]() -> int {
    if (!ctx || !count || !npts || (!idx && max) || (!pts && max_pts)) return BZH_E_ARG;
    auto &s = ctx->strm;
    *count = 0;
    *npts = 0;
    if (!s.index) {
        bzh_set_error(ctx, "stream index: the stream was not begun with bzh_stream_begin_index");
        return BZH_E_STATE;
    }
    if (!bzs_take(s.ix_entries, s.ix_pts, idx, max, count, pts, max_pts, npts)) {
        bzh_set_error(ctx, "stream index: %zu entries and %zu sync points pending, room for %zu and %zu", *count, *npts, max, max_pts);
        return BZH_E_CAP;
    }
    return BZH_OK;
    });
}

// ---- index files: host only, no context (stream_index.h) -------------------------------------------------------------------
extern "C" size_t bzh_index_blob_size(size_t count, size_t npts, uint32_t interval) { return bzs_blob_size(count, npts, interval); }

extern "C" int bzh_index_blob_write(const bzh_index_entry *idx, size_t count, const bzh_sync_point *pts, size_t npts, uint32_t interval,
                                    uint64_t consumed, uint8_t *out, size_t cap, size_t *out_len)
{
    return bzs_blob_write(idx, count, pts, npts, interval, consumed, out, cap, out_len);
}

extern "C" int bzh_index_blob_read(const uint8_t *blob, size_t n, bzh_index_entry *idx, size_t max, size_t *count, bzh_sync_point *pts,
                                   size_t max_pts, size_t *npts, uint32_t *interval, uint64_t *consumed)
{
    return bzs_blob_read(blob, n, idx, max, count, pts, max_pts, npts, interval, consumed);
}

extern "C" size_t bzh_stream_bound(const bzh_ctx *ctx, size_t n)
{
    if (!ctx) return 0;
    // everything not yet handed out may be released by this call: the pass in flight, the bytes waiting
    // for the next pass, n, and a carried tail (< 52 MB: one block of a maximal run), at worst-case
    // expansion, plus framing
    const auto &s = ctx->strm;
    const size_t raw = n + s.pending + (s.inflight ? s.pass.total : 0) + ((size_t)52 << 20);
    return raw + raw / 4 + (raw / 70000 + 4) * 4096 + 65536;
}

extern "C" size_t bzh_stream_consumed(const bzh_ctx *ctx) { return ctx ? ctx->strm.consumed : 0; }

extern "C" int bzh_stream_set_chunk(bzh_ctx *ctx, size_t bytes)
{
    return bzh_guard(ctx, [&]() -> int {
    if (!ctx || bytes == 0 || bytes > ((size_t)1 << 30)) return BZH_E_ARG;
    ctx->strm.min_feed = bytes;
    return BZH_OK;
    });
}

// Headroom kept in front of the fed bytes for the tail a pass leaves unconsumed (normally well below
// one block of raw input; larger tails -- a block inside one enormous run -- regrow the buffer).
static const size_t STREAM_HEAD = (size_t)4 << 20;

// Makes d_buf[fill] hold `head` bytes of headroom + the pending bytes + `extra` more, keeping the
// pending bytes.
static int stream_reserve(bzh_ctx *ctx, size_t head, size_t extra)
{
    auto &s = ctx->strm;
    const int f = s.fill;
    if (s.d_buf[f] && head <= s.head && s.head + s.pending + extra + 16 <= s.d_buf[f].cap) return BZH_OK;
    const size_t nhead = align_up(std::max(head, std::max(s.head, STREAM_HEAD)), 4096);
    const size_t want = align_up(nhead + std::max(s.pending + extra, s.min_feed) + ((size_t)16 << 20), 4096);
    DevBuf nb; // (a fresh one: the pending bytes move over on the copy stream, the pass in flight on ctx->stream is not waited for)
    BZH_TRY(nb.reserve(ctx, want, "the fed bytes of a stream"));
    if (s.pending) HIP_TRY(ctx, hipMemcpyAsync(nb.p + nhead, s.d_buf[f].p + s.head, s.pending, hipMemcpyDeviceToDevice, s.copy_stream));
    HIP_TRY(ctx, bzh_stream_wait(s.copy_stream));
    std::swap(nb.p, s.d_buf[f].p), std::swap(nb.cap, s.d_buf[f].cap);
    s.head = nhead;
    return BZH_OK;
}

// The pass in flight, on its own thread: split, encode the blocks whose cut cannot move any more,
// bring their bits to pinned host memory.  Touches the context's plan / batch state and ctx->stream
// only; the feeding thread meanwhile uses the other buffer and the copy stream.
static void stream_pass(bzh_ctx *ctx)
{
    auto &s = ctx->strm;
    auto &p = s.pass;
    p.used = 0;
    p.nbits = 0;
    p.out_bytes = 0;
    p.lastw = 0;
    p.crcs.clear();
    p.entries.clear();
    p.pts.clear();
    p.rc = bzh_guard(ctx, [&]() -> int {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        const uint8_t *buf = s.d_buf[p.buf] + p.off;
        BZH_TRY(rle1_plan(ctx, buf, p.total, true, true));
        const size_t nb = ctx->plan_blocks.size();
        size_t F = nb; // blocks that are final
        if (!p.eof) {
            F = 0;
            while (F < nb && !ctx->plan_open[F]) F++;
        }
        if (F == 0) return BZH_OK;
        p.used = F == nb ? p.total : (size_t)ctx->plan_blocks[F].in_off;
        size_t raw = 0;
        for (size_t k = 0; k < F; k++) raw += ctx->plan_blocks[k].in_len;
        const size_t dcap = (raw + raw / 4 + (F + 2) * 4096 + 65536) & ~(size_t)3;
        BZH_TRY(ensure_stage(ctx, s.d_out[p.obuf], dcap));
        uint8_t *d_o = s.d_out[p.obuf];
        uint8_t seed_be[4];
        put_be32(seed_be, p.seed);
        uint32_t seed;
        memcpy(&seed, seed_be, 4);
        stats_begin(ctx);
        EncIndex ix{s.interval, {}, {}};
        if (s.index) BZH_TRY(rle1_plan_crc_join(ctx)); // (the entries carry the block CRCs, as in encode_device_impl)
        BZH_TRY(encode_range(ctx, 0, F, d_o, s.d_out[p.obuf].cap & ~(size_t)3, p.phase, &p.nbits, p.phase ? &seed : nullptr, nullptr,
                             s.index ? &ix : nullptr));
        p.entries.swap(ix.entries);
        p.pts.swap(ix.pts);
        const uint64_t bits_in_buf = p.phase + p.nbits;
        const size_t full_words = (size_t)(bits_in_buf / 32);
        BZH_TRY(s.h_out.reserve(ctx, 4096, "a pass's last word"));
        // the whole words stay on the device until the caller's next feed collects them; only the partial word behind
        // them (it seeds the next pass) comes back now
        if (bits_in_buf & 31u) HIP_TRY(ctx, hipMemcpyAsync(s.h_out, d_o + full_words * 4, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, bzh_stream_wait(st));
        p.out_bytes = full_words * 4;
        if (bits_in_buf & 31u) {
            const uint8_t *w = s.h_out;
            p.lastw = ((uint32_t)w[0] << 24) | ((uint32_t)w[1] << 16) | ((uint32_t)w[2] << 8) | w[3];
        }
        BZH_TRY(rle1_plan_crc_join(ctx));
        for (size_t k = 0; k < F; k++) p.crcs.push_back(ctx->plan_blocks[k].crc);
        return BZH_OK;
    });
}

extern "C" int bzh_stream_feed(bzh_ctx *ctx, const uint8_t *in, size_t n, int eof, uint8_t *out, size_t cap,
                               size_t *out_len)
{
    return bzh_guard(ctx, [&]() -> int {
    if (!ctx || (!in && n) || !out || !out_len) return BZH_E_ARG;
    auto &s = ctx->strm;
    if (!s.active) return BZH_E_STATE;
    *out_len = 0;
    const size_t PIECE = (size_t)256 << 20; // keeps every plan far inside 32-bit positions
    if (n > PIECE) {
        size_t done = 0, produced = 0;
        while (done < n) {
            const size_t k = n - done < PIECE ? n - done : PIECE;
            size_t got = 0;
            BZH_TRY(bzh_stream_feed(ctx, in + done, k, eof && done + k == n, out + produced, cap - produced, &got));
            done += k;
            produced += got;
        }
        *out_len = produced;
        return BZH_OK;
    }
    if (cap < bzh_stream_bound(ctx, n)) return BZH_E_CAP; // before anything is consumed: the call can be repeated
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!s.copy_stream) HIP_TRY(ctx, hipStreamCreateWithFlags(&s.copy_stream, hipStreamNonBlocking));

    // 1. the fed bytes go straight to the device, behind what is already waiting there; this runs
    //    while the previous pass (if any) is still encoding
    if (n) {
        BZH_TRY(stream_reserve(ctx, s.head, n));
        HIP_TRY(ctx, hipMemcpyAsync(s.d_buf[s.fill] + s.head + s.pending, in, n, hipMemcpyHostToDevice, s.copy_stream));
        HIP_TRY(ctx, bzh_stream_wait(s.copy_stream)); // `in` belongs to the caller again on return
        s.pending += n;
    }
    if (!eof && s.pending < s.min_feed) return BZH_OK;

    size_t opos = 0;
    if (!s.header_done) { // lib/lib.rs:18-22
        out[0] = 0x42;
        out[1] = 0x5A;
        out[2] = 0x68;
        out[3] = (uint8_t)('0' + ctx->level);
        opos = 4;
        s.bitpos = 32;
        s.header_done = true;
    }
    // 2. take the results of the pass in flight: its bits are final now
    size_t left = 0;
    const uint8_t *tail = nullptr;
    struct Done {
        int obuf;
        size_t bytes;
    } done[2];
    int ndone = 0;
    // the finished passes' words: device -> the caller's buffer (called with the next pass already running)
    // (A failure here loses words whose bits are already counted in bitpos / carry_word / stream_crc: the stream cannot go
    // on -- later feeds get BZH_E_STATE, not a stream with a hole.)
    auto drain = [&]() -> int {
        const int rc = [&]() -> int {
            for (int k = 0; k < ndone; k++) {
                HIP_TRY(ctx, hipMemcpyAsync(out + opos, s.d_out[done[k].obuf], done[k].bytes, hipMemcpyDeviceToHost, s.copy_stream));
                opos += done[k].bytes;
            }
            if (ndone) HIP_TRY(ctx, bzh_stream_wait(s.copy_stream));
            return BZH_OK;
        }();
        ndone = 0;
        if (rc != BZH_OK) s.active = false;
        return rc;
    };
    auto collect = [&]() -> int {
        stream_join(ctx);
        s.inflight = false;
        const auto &p = s.pass;
        if (p.rc != BZH_OK) {
            s.active = false;
            return p.rc;
        }
        if (p.out_bytes) done[ndone++] = {p.obuf, p.out_bytes};
        if (s.index && !p.entries.empty()) { // the pass's entries and points, in stream coordinates, behind what is pending
            const size_t e0 = s.ix_entries.size(), p0 = s.ix_pts.size();
            s.ix_entries.insert(s.ix_entries.end(), p.entries.begin(), p.entries.end());
            s.ix_pts.insert(s.ix_pts.end(), p.pts.begin(), p.pts.end());
            bzs_rebase(bzs_base(s.bitpos, s.consumed, s.ix_blocks), s.ix_entries.data() + e0, p.entries.size(), s.ix_pts.data() + p0,
                       p.pts.size());
            s.ix_blocks += p.entries.size();
        }
        if (p.nbits) {
            s.carry_word = p.lastw;
            s.bitpos += p.nbits;
        }
        for (uint32_t c : p.crcs) s.stream_crc = c ^ ((s.stream_crc << 1) | (s.stream_crc >> 31)); // lib/lib.rs:107-108
        s.consumed += p.used;
        left = p.total - p.used;
        tail = s.d_buf[p.buf] + p.off + p.used;
        return BZH_OK;
    };
    if (s.inflight) BZH_TRY(collect());

    // 3. start the next pass on [tail of the previous pass | fed bytes]
    for (;;) {
        const size_t total = left + s.pending;
        if (total == 0) break;
        BZH_TRY(stream_reserve(ctx, left, 0));
        if (left) {
            HIP_TRY(ctx, hipMemcpyAsync(s.d_buf[s.fill] + s.head - left, tail, left, hipMemcpyDeviceToDevice, s.copy_stream));
            HIP_TRY(ctx, bzh_stream_wait(s.copy_stream));
        }
        auto &p = s.pass;
        p.buf = s.fill;
        p.off = s.head - left;
        p.total = total;
        p.eof = eof != 0;
        p.phase = (uint32_t)(s.bitpos & 31u);
        p.seed = s.carry_word;
        p.obuf = s.osel;
        s.osel ^= 1;
        s.inflight = true;
        s.worker = std::thread(stream_pass, ctx);
        s.fill ^= 1; // the other buffer is free: its pass was collected above, its tail copied
        s.head = STREAM_HEAD;
        s.pending = 0;
        BZH_TRY(drain()); // (the pass before this one: its output buffer is the one the pass after this one will use)
        if (!eof) break;
        // 4. end of input: wait for this last pass too (it consumes everything it was given)
        left = 0;
        BZH_TRY(collect());
        if (left == 0) break; // always, at eof; the loop guards against a pass that could not finish its tail
    }
    BZH_TRY(drain());

    if (eof) { // footer + stream CRC (lib/lib.rs:66-70), zero padding to a byte (lib/out.rs:22-28)
        const uint32_t phase = (uint32_t)(s.bitpos & 31u);
        uint8_t tailb[24];
        memset(tailb, 0, sizeof tailb);
        put_be32(tailb, phase ? s.carry_word : 0u);
        const uint8_t foot[10] = {0x17, 0x72, 0x45, 0x38, 0x50, 0x90, (uint8_t)(s.stream_crc >> 24),
                                  (uint8_t)(s.stream_crc >> 16), (uint8_t)(s.stream_crc >> 8), (uint8_t)s.stream_crc};
        for (uint32_t k = 0; k < 80; k++) {
            const uint32_t bit = (foot[k >> 3] >> (7 - (k & 7))) & 1u;
            const uint32_t pos = phase + k;
            tailb[pos >> 3] |= (uint8_t)(bit << (7 - (pos & 7)));
        }
        const size_t nbytes = (phase + 80 + 7) / 8;
        memcpy(out + opos, tailb, nbytes);
        opos += nbytes;
        s.bitpos += 80;
        s.active = false;
        // (the two input buffers stay with the context for its next stream -- bzh_destroy frees them: a hipMalloc of 150 MB at
        // the first feed and two synchronizing hipFree at the end were 0.3-0.5 ms of every stream of the API path)
        s.head = 0;
    }
    *out_len = opos;
    return BZH_OK;
    });
}
