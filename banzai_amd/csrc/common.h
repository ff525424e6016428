// common.h -- shared declarations of libbzhip.so (MI355X / gfx950 only).
// Context, workspace arena, error plumbing and the wavefront-64 scan primitives every stage uses.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/bzhip.h"

#define BZH_WAVE 64

// ---- error plumbing -----------------------------------------------------------------------
struct bzh_ctx;
void bzh_set_error(bzh_ctx *ctx, const char *fmt, ...);

#define HIP_TRY(ctx, expr)                                                                         \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            bzh_set_error((ctx), "%s:%d %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e_)); \
            return BZH_E_HIP;                                                                      \
        }                                                                                          \
    } while (0)

// Waits for a stream.  The suffix-sort rounds no longer wait for the host (bwt.hip), so a batch is left with a
// handful of waits (block table, bit totals, end of the pack): a short poll catches the ones that are about to
// complete, then the thread blocks in hipStreamSynchronize instead of spinning on a core.
static inline hipError_t bzh_stream_wait(hipStream_t st)
{
    for (unsigned it = 0; it < 256u; it++) {
        const hipError_t e = hipStreamQuery(st);
        if (e != hipErrorNotReady) return e;
    }
    return hipStreamSynchronize(st);
}

#define BZH_TRY(expr)                                                                              \
    do {                                                                                           \
        int s_ = (expr);                                                                           \
        if (s_ != BZH_OK) return s_;                                                               \
    } while (0)

// ---- grow-only buffers ---------------------------------------------------------------------------------------------------
// Memory a context keeps between calls and only ever grows: device memory, or pinned host memory (PinnedBuf).  reserve() is the
// one place that allocates: nothing happens while the capacity suffices; otherwise the context's stream is waited for, the old
// allocation freed and `grow(need)` bytes -- `need` itself without a policy -- allocated.  On failure the buffer is left empty,
// the error text names `what`, BZH_E_NOMEM comes back.  The destructor frees (bzh_destroy makes the device current first).
static inline size_t grow_eighth(size_t need) { return (need + need / 8 + 4096 + 4095) / 4096 * 4096; } // staging: a stream of growing calls does not reallocate every time
static inline size_t grow_mib(size_t need) { return (need + 0xFFFFF) & ~(size_t)0xFFFFF; }               // the sync-point recorder
static inline size_t grow_double(size_t need) { return need * 2; }                                        // the pinned landing place of the block CRCs
template <bool PINNED>
struct GrowBuf {
    uint8_t *p = nullptr;
    size_t cap = 0;
    unsigned flags = 0; // PinnedBuf: hipHostMalloc flags
    GrowBuf() = default;
    GrowBuf(GrowBuf &&o) noexcept : p(o.p), cap(o.cap), flags(o.flags) { o.p = nullptr, o.cap = 0; }
    ~GrowBuf() { release(); }
    int reserve(bzh_ctx *ctx, size_t need, const char *what, size_t (*grow)(size_t) = nullptr); // (ctx may be null: no stream to wait for, no text)
    void release() { if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p)); p = nullptr, cap = 0; }
    template <typename T>
    T *as() const { return reinterpret_cast<T *>(p); }
    operator uint8_t *() const { return p; }
};
using DevBuf = GrowBuf<false>;
using PinnedBuf = GrowBuf<true>;

#include "search_plan.h" // the windows of a search and their carry: host-only text (tests/decode_host/search_host.cpp)
#include "grep_plan.h" // the windows of a grep and their carry: host-only text (tests/decode_host/grep_host.cpp)
#include "grep_ctx_plan.h" // ... with context records (tests/decode_host/grep_ctx_host.cpp)
#include "match_plan.h" // the windows of bzh_match* and the cursor between them (tests/decode_host/match_host.cpp)
#include "batch.h" // geometry, Batch and its layout, the carver: host-only text (tests/workspace_host)

// Kernel classes of the per-kernel roofline table (bzh_get_kernel_stats).  With profiling on, the launches of a
// class are bracketed by HIP events on the context's stream (KSpan); `bytes` = ALGORITHMIC bytes the launches move
// (per-element figures in DESIGN.md, element counts from the plan / the round summaries).
enum KClass : int {
    K_PLAN = 0, K_CRC, K_RLE1_EMIT, K_BYTE_COUNT, K_RADIX_INIT, K_RADIX_GID, K_REFINE_INIT, K_RANK_APPLY,
    K_ROUND_BEGIN, K_SWEEP, K_ACTIVE_GEN, K_RADIX_ROUNDS, K_TAIL_ROUND, K_REFINE_ROUNDS, K_BWT_EMIT, K_MTF_LAST,
    K_MTF_WALK, K_HUFF, K_PACK, K_MSD_PLAN, K_MSD_SCATTER, K_MSD_LEVELS, K_MSD_FINISH, K_MID_SORT, K_COUNT
};
static const char *const KCLASS_NAME[K_COUNT] = {
    "plan (granules, carries, split)", "crc_tiles", "rle1_emit", "byte_count", "radix_scatter (initial sort)",
    "radix_scatter<GID> (re-key pass)", "refine_one<init> (+ rank binning)", "rank_apply", "round_begin",
    "SWEEP path (3 passes + 3-kernel refine)", "active_gen", "radix_scatter (big-list rounds)", "tail_round",
    "refine_one (rounds)", "bwt_emit", "mtf_tile_last + mtf_prefix (+ RLE2 layout)", "mtf_walk (+ RLE2 emit)",
    "huffman (segments, build, header)", "pack_symbols", "bigram_hist + bigram_plan", "bigram_scatter (2-byte buckets)",
    "seg_count/plan/scatter (oversized buckets)", "chunk_finish (bucket sort + ranks in LDS)",
    "mid_sort (round 0: large groups in LDS)"};

struct Timer {
    hipEvent_t a = nullptr, b = nullptr;
};

// ---- many inputs, one stream each (bzh_encode_many*) ------------------------------------------------------------
// Stream k lies at byte offs[k] of the output, offs[k+1] = align4(offs[k] + lens[k]).  A stream may span several batches, so the
// layout is carried from batch to batch in a small device record (many_layout writes it, the next batch's many_layout reads it).
enum ManyState : int {
    MST_OFF = 0, // byte offset of the stream the next batch continues or starts (input ManyBatch::lo)
    MST_BODY,    // its body bits so far (0: not started)
    MST_CRC,     // its partial CRC fold (crc = block ^ rotl(crc, 1), lib/lib.rs:107-108)
    MST_ZEROED,  // first output word not yet zeroed
    MST_OVER,    // 1: some batch did not fit the output (every later pack is gated off)
    MST_BITS,    // block bits written so far (bzh_stats::out_bits)
    MST_Z0,      // this batch zeroes words [Z0, Z1)
    MST_Z1,
    MST_WORDS    // (record size in 64-bit words)
};
struct ManyOut { // device arrays of a call over many inputs: state | offs | lens | body | crc (state, offs, lens: ONE copy back)
    uint64_t *state; // [MST_WORDS]
    uint64_t *offs;  // [count] byte offset of every stream
    uint64_t *lens;  // [count] bytes of every stream
    uint64_t *body;  // [count] body bits of every stream complete so far (0 for an empty one)
    uint32_t *crc;   // [count] its stream CRC
};
struct ManyBatch { // what the plan tells the host about a batch (kernel argument)
    uint32_t B;          // blocks
    uint32_t lo;         // the first input the batch places: the stream it continues or the next one to start
    uint32_t close_hi;   // inputs [lo, close_hi) are complete behind this batch (offsets, lengths, footers)
    uint32_t hi;         // inputs [lo, hi) get their offsets: close_hi + 1 while the batch's last stream stays open
    uint32_t lo_started; // 1: input lo's header was written by an earlier batch
    uint32_t level;
    uint64_t cap_words;  // output capacity in 32-bit words
};

struct bzh_ctx {
    bzh_ctx *parent = nullptr;        // lanes: the context that owns the plan and the arena
    std::vector<bzh_ctx *> lanes;     // two half-batch workers (own stream, half of the arena each)
    int nlanes = 1;                   // 1: batches run one after the other on this context; 2: on the lanes
    int device = 0;
    int level = 9;
    uint32_t M = 0;
    uint32_t S = 0;
    uint32_t max_batch = 0;
    hipStream_t stream = nullptr;
    hipStream_t side_stream = nullptr;   // second stream of the suffix sort (big-list path beside the small groups)
    hipStream_t side2_stream = nullptr;  // third stream: the global passes of the blocks mid_sort does not take, beside it (rounds >= 1)
    hipEvent_t side_ev[3] = {nullptr, nullptr, nullptr};
    // the plan's work beside the main stream (rle1.hip): the block CRCs -- nothing needs them before the block headers are
    // written -- and the table prefetch of the split run on the second stream between these events
    hipEvent_t plan_ev[2] = {nullptr, nullptr};
    bool crc_pending = false;           // the CRCs of the current plan are on their way (rle1_plan_crc_join collects them)
    PinnedBuf crc_host;                 // their landing place: PINNED (a copy to pageable memory holds the host until it is done)
    size_t crc_host_len = 0;
    int profiling = 0;
    int mode = 0;                     // BZH_MODE_REFERENCE / BZH_MODE_FIXED (bzh_set_mode)
    char err[512] = {0};      // last failure (guarded by err_mu: the streaming worker writes it too)
    char err_out[512] = {0};  // copy handed out by bzh_last_error
    std::mutex err_mu;
    // arena
    DevBuf arena;
    uint32_t arena_blocks = 0;        // blocks per batch the arena is laid out for (ensure_arena, api.hip)
    Batch bt{};
    // plan
    const uint8_t *plan_in = nullptr; // device
    size_t plan_n = 0;
    uint32_t wgflag = 0;                // WG_SPREAD for the launches of the current group when few blocks are active
    std::vector<bzh_block> plan_blocks;
    std::vector<uint8_t> plan_open;     // per block: 1 = cut not final unless the input ends here
    std::vector<uint8_t> plan_host;     // host copy of the plan's device records (scratch of rle1_plan)
    std::vector<uint8_t> plan_crc_ok;   // per block: CRC computed (bzh_plan_device_nocrc leaves them to the encoder)
    DevBuf plan_ws;                     // device scratch of the plan (run tables)
    uint32_t plan_extra = 0;            // block records the plan holds beyond one stream's bound (a plan of many inputs: one an input)
    std::vector<uint32_t> plan_input;   // a plan of many inputs: the input of every block (empty for a plan of one buffer)
    // many inputs (bzh_encode_many*, rle1_plan_many)
    DevBuf many_ws;                     // device: guarded input buffer, input table, split records, block -> input
    uint32_t *many_binp = nullptr;      // [blocks] input of every block of the plan (in many_ws)
    std::vector<uint32_t> many_tab;     // host copy of the input table (source of an async copy: lives in the context)
    DevBuf many_out;                    // device: ManyOut arrays
    std::vector<uint64_t> many_host;    // state | offs | lens read back at the end of a call
    std::vector<uint8_t> many_pack;     // bzh_encode_many: the host inputs back to back (one H2D)
    // staging
    DevBuf d_stage_in, d_stage_out;
    PinnedBuf h_pinned;           // small pinned readback area: pinned_words(max_batch) 32-bit words (pinned_alloc, api.hip)
    DevBuf d_crctab;              // GF(2) tables of the block CRC (rle1.hip)
    // decode (decode.hip): allocated by the first decode, so an encode-only user pays nothing
    DevBuf dec_ws;                // per-batch tables: candidates, results, tile maps / counts / offsets, CRC descriptors
    DevBuf dec_list;              // the scan's hit list (64-bit words)
    DevBuf sync_ws;               // sync points (allocated on first use): the recorder's slots, a range's headers, points and segments, or an encoded batch's points
    bzh_decode_stats dstats{};
    bzh_decode_many_stats mstats{}; // of the last bzh_decode_many* call
    bzh_recover_stats rstats{};     // of the last bzh_recover* call
    bzh_decode_ranges_stats qstats{}; // of the last bzh_decode_ranges* call
    DevBuf ranges_ws;               // bzh_decode_ranges*: a batch's piece tables (allocated on first use)
    DevBuf records_ws;              // records (bzh_decode_index_records*, bzh_decode_records*, bzh_count_records_device): tile counts, last-byte flags, queries, positions
    DevBuf search_ws;               // bzh_search*, bzh_grep*: the staging buffer the decoders expand a window into (allocated on first use)
    DevBuf scan_carry;              // ... and what is carried from one window to the next: the last plen - 1 bytes, or a grep's open record
    DevBuf search_tab, search_out;  // bzh_search*: a window's tile tables, its hit slots
    size_t search_room = 0;         // bzh_search_set_room: the staging target of the range search (0: the default)
    bzh_search_stats sstats{};      // of the last bzh_search* call
    DevBuf grep_tab, grep_ent;      // bzh_grep*: a window's tile tables, its entries
    bzh_grep_stats gstats{};        // of the last bzh_grep* call
    bzh_grep_context_stats gcstats{};
    uint32_t grep_before = 0, grep_after = 0; // bzh_grep_set_context
    DevBuf grep_many_tab;             // bzh_grep_many*: the segment table, the virtual tile table, the segments' totals
    bzh_grep_many_stats gmstats{};    // of the last bzh_grep_many* call
    DevBuf match_tab, match_ent;    // bzh_match*: a window's tile tables, its entries
    bzh_match_stats mtstats{};      // of the last bzh_match* call
    struct DStream *dstrm = nullptr; // streaming decode (bzh_dstream_*, decode.hip): made by the first begin, freed by dstream_free
    size_t dstrm_window = 0, dstrm_staging = 0; // bzh_dstream_set_room: targets of the next begin (0: the defaults)
    // streaming encode (bzh_stream_*)
    struct Stream {
        bool active = false, header_done = false;
        // Two device buffers.  d_buf[fill] receives the fed bytes from offset `head` on (copy stream);
        // when a pass starts, the unconsumed tail of the previous pass is placed right before `head`,
        // so the pass sees one contiguous range.  The previous pass's buffer is free again by then.
        DevBuf d_buf[2];
        int fill = 0;
        size_t head = 0;                // offset of the first fed byte in d_buf[fill]
        size_t pending = 0;             // fed bytes waiting in d_buf[fill]
        uint64_t bitpos = 0;            // stream bits handed out or in `carry_word`
        uint32_t carry_word = 0;        // the bitpos % 32 bits not yet handed out (big-endian word)
        uint32_t stream_crc = 0;
        size_t consumed = 0;
        size_t min_feed = (size_t)32 << 20; // pending bytes that trigger a GPU pass
        hipStream_t copy_stream = nullptr;  // H2D of fed bytes, concurrent with the pass in flight
        // the pass in flight (worker thread): plan + encode + D2H of its final blocks
        std::thread worker;
        bool inflight = false;
        struct Pass {
            int buf = 0;                // which d_buf
            int obuf = 0;               // which d_out
            size_t off = 0, total = 0;  // input range of the pass
            bool eof = false;
            uint32_t phase = 0, seed = 0; // bit phase / carried bits at the start of the pass
            // results
            int rc = 0;
            size_t used = 0;            // input bytes consumed by the final blocks
            uint64_t nbits = 0;
            size_t out_bytes = 0;       // whole words copied to h_out
            uint32_t lastw = 0;         // the partial word after them (big-endian value)
            std::vector<uint32_t> crcs; // CRCs of the final blocks, in order
            std::vector<bzh_index_entry> entries; // an indexed stream: the final blocks' entries and sync points, in the
            std::vector<bzh_sync_point> pts;      // PASS's coordinates (the feed that collects the pass rebases them: stream_index.h)
        } pass;
        // bzh_stream_begin_index: the stream records its index.  What the collected passes found waits here, in stream
        // coordinates, until bzh_stream_index_take moves it out (kept after a failure and after eof, dropped by the next begin).
        bool index = false;
        uint32_t interval = 0;
        std::vector<bzh_index_entry> ix_entries;
        std::vector<bzh_sync_point> ix_pts;
        uint64_t ix_blocks = 0;         // blocks of the collected passes: taken + pending
        PinnedBuf h_out;                // pinned: the partial last word of a pass's output
        // A pass leaves its bits on the device (two buffers, alternating): the next pass is started first, then the
        // finished one's words go straight to the caller's buffer while the GPU is already at work again.
        DevBuf d_out[2];
        int osel = 0;
    } strm;
    bzh_stats stats{};
    uint32_t debug_fault = 0;         // bzh_debug_fault: fault to inject into the next suffix sort
    bool no_spread = false;           // look-back kernels keep every block on one XCD (set for good after a look-back gave up: bwt_run)
    uint32_t bwt_epoch = 0;           // suffix-sort attempts so far (SortAttempt: tags the round summaries in pinned memory)
    std::vector<hipEvent_t> evpool;
    size_t evnext = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> sort_spans;
    struct KRec { int cls; hipEvent_t a, b; };
    std::vector<KRec> kspans;          // profiling: event pairs per kernel class of the call in flight
    uint64_t k_cur_ntotal = 0;         // RLE1 bytes of the batch in flight (byte counts of the stages around the sort)
    double k_ms[K_COUNT] = {0};        // collected by kstats_collect
    uint64_t k_bytes[K_COUNT] = {0}, k_launch[K_COUNT] = {0};
};

template <bool PINNED>
int GrowBuf<PINNED>::reserve(bzh_ctx *ctx, size_t need, const char *what, size_t (*grow)(size_t))
{
    if (need <= cap) return BZH_OK;
    if (p) {
        if (ctx) HIP_TRY(ctx, bzh_stream_wait(ctx->stream));
        release();
    }
    const size_t want = grow ? grow(need) : need;
    if ((PINNED ? hipHostMalloc((void **)&p, want, flags) : hipMalloc((void **)&p, want)) != hipSuccess) {
        p = nullptr;
        bzh_set_error(ctx, "%s(%zu) for %s failed", PINNED ? "hipHostMalloc" : "hipMalloc", want, what);
        return BZH_E_NOMEM;
    }
    cap = want;
    return BZH_OK;
}

// A buffer reserved for, and cut into, the arrays `cut` takes from the carver it is given: a measuring pass sizes it, a second one cuts.
template <typename F>
static inline int reserve_cut(bzh_ctx *ctx, DevBuf &buf, const char *what, size_t (*grow)(size_t), F cut)
{
    Carver measure(nullptr);
    cut(measure);
    BZH_TRY(buf.reserve(ctx, measure.bytes(), what, grow));
    Carver carve(buf.p);
    cut(carve);
    return BZH_OK;
}

// words of a context's pinned readback area: 8 a block and 64 free ones (api.hip), the round summaries and the initial sort's plan record (bwt.hip)
static inline size_t pinned_words(uint32_t max_batch) { return (size_t)max_batch * 8 + 64 + (size_t)(MAX_ROUNDS + 1) * SUMMARY_WORDS; }

hipEvent_t bzh_event(bzh_ctx *ctx);
// Brackets the launches issued during its lifetime (one class) with events when profiling is on.
struct KSpan {
    bzh_ctx *c;
    int cls;
    hipEvent_t a = nullptr;
    KSpan(bzh_ctx *ctx, int k, uint64_t bytes, uint64_t launches = 1) : c(ctx), cls(k)
    {
        if (!c->profiling) return;
        a = bzh_event(c);
        hipEventRecord(a, c->stream);
        c->k_bytes[k] += bytes;
        c->k_launch[k] += launches;
    }
    ~KSpan()
    {
        if (!a) return;
        hipEvent_t b = bzh_event(c);
        hipEventRecord(b, c->stream);
        c->kspans.push_back({cls, a, b});
    }
};

// ---- wavefront-64 primitives ----------------------------------------------------------------
__device__ __forceinline__ uint32_t run_digits(uint32_t z) // symbols emitted for a zero run of length z
{
    return z ? (31u - __clz(z + 1u)) : 0u;
}

__device__ __forceinline__ uint32_t wave_incl_add(uint32_t v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint32_t t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

__device__ __forceinline__ int wave_incl_max(int v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        int t = __shfl_up(v, d, 64);
        if (lane >= d) v = max(v, t);
    }
    return v;
}

__device__ __forceinline__ uint32_t wave_reduce_add(uint32_t v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// Wavefront reductions without address registers: five ds_swizzle steps (the xor pattern is an immediate) and two lane
// reads.  The __shfl_xor forms above cost six lane-dependent addresses, which a kernel that loops over work items keeps alive
// across the whole loop -- in a kernel at its register limit that is six registers in scratch memory.  Result in every lane.
#define BZH_SWZ(v, x) __builtin_amdgcn_ds_swizzle((int)(v), ((x) << 10) | 0x1F)
__device__ __forceinline__ uint32_t wave_all_add(uint32_t v)
{
    v += (uint32_t)BZH_SWZ(v, 1);
    v += (uint32_t)BZH_SWZ(v, 2);
    v += (uint32_t)BZH_SWZ(v, 4);
    v += (uint32_t)BZH_SWZ(v, 8);
    v += (uint32_t)BZH_SWZ(v, 16);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 0) + (uint32_t)__builtin_amdgcn_readlane((int)v, 32);
}
__device__ __forceinline__ uint32_t wave_all_max(uint32_t v)
{
    v = max(v, (uint32_t)BZH_SWZ(v, 1));
    v = max(v, (uint32_t)BZH_SWZ(v, 2));
    v = max(v, (uint32_t)BZH_SWZ(v, 4));
    v = max(v, (uint32_t)BZH_SWZ(v, 8));
    v = max(v, (uint32_t)BZH_SWZ(v, 16));
    return max((uint32_t)__builtin_amdgcn_readlane((int)v, 0), (uint32_t)__builtin_amdgcn_readlane((int)v, 32));
}
__device__ __forceinline__ uint32_t wave_all_or(uint32_t v)
{
    v |= (uint32_t)BZH_SWZ(v, 1);
    v |= (uint32_t)BZH_SWZ(v, 2);
    v |= (uint32_t)BZH_SWZ(v, 4);
    v |= (uint32_t)BZH_SWZ(v, 8);
    v |= (uint32_t)BZH_SWZ(v, 16);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 0) | (uint32_t)__builtin_amdgcn_readlane((int)v, 32);
}
__device__ __forceinline__ uint32_t wave_all_and(uint32_t v)
{
    v &= (uint32_t)BZH_SWZ(v, 1);
    v &= (uint32_t)BZH_SWZ(v, 2);
    v &= (uint32_t)BZH_SWZ(v, 4);
    v &= (uint32_t)BZH_SWZ(v, 8);
    v &= (uint32_t)BZH_SWZ(v, 16);
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 0) & (uint32_t)__builtin_amdgcn_readlane((int)v, 32);
}

// Inclusive OR-scan over the 64 lanes by data-parallel primitives (no lane addresses, no compares): four shifts inside the
// rows of 16 (a lane without a source reads 0), then the last lane of a row to the rows behind it.  OR is idempotent, so
// the plain doubling needs no bank masks.
#define BZH_DPP_OR(v, ctrl, rowmask) ((v) | (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(v), (ctrl), (rowmask), 0xF, true))
__device__ __forceinline__ uint32_t wave_incl_or(uint32_t v)
{
    v = BZH_DPP_OR(v, 0x111, 0xF); // row_shr:1
    v = BZH_DPP_OR(v, 0x112, 0xF); // row_shr:2
    v = BZH_DPP_OR(v, 0x114, 0xF); // row_shr:4
    v = BZH_DPP_OR(v, 0x118, 0xF); // row_shr:8
    v = BZH_DPP_OR(v, 0x142, 0xA); // row_bcast:15 -> rows 1 and 3
    v = BZH_DPP_OR(v, 0x143, 0xC); // row_bcast:31 -> rows 2 and 3
    return v;
}
// The same doubling for sums and for unsigned maxima (a lane without a source reads 0, the identity of both): inside a row
// the shifted adds are the plain inclusive scan, then rows 1 and 3 take the total of the row before them, then rows 2 and 3
// the total of rows 0-1.  Six vector instructions, no LDS crossbar: what a kernel bound by instruction issue wants.
#define BZH_DPP_SRC(v, ctrl, rowmask) ((uint32_t)__builtin_amdgcn_update_dpp(0, (int)(v), (ctrl), (rowmask), 0xF, true))
__device__ __forceinline__ uint32_t wave_incl_add_dpp(uint32_t v)
{
    v += BZH_DPP_SRC(v, 0x111, 0xF);
    v += BZH_DPP_SRC(v, 0x112, 0xF);
    v += BZH_DPP_SRC(v, 0x114, 0xF);
    v += BZH_DPP_SRC(v, 0x118, 0xF);
    v += BZH_DPP_SRC(v, 0x142, 0xA);
    v += BZH_DPP_SRC(v, 0x143, 0xC);
    return v;
}
__device__ __forceinline__ uint32_t wave_incl_umax_dpp(uint32_t v)
{
    v = max(v, BZH_DPP_SRC(v, 0x111, 0xF));
    v = max(v, BZH_DPP_SRC(v, 0x112, 0xF));
    v = max(v, BZH_DPP_SRC(v, 0x114, 0xF));
    v = max(v, BZH_DPP_SRC(v, 0x118, 0xF));
    v = max(v, BZH_DPP_SRC(v, 0x142, 0xA));
    v = max(v, BZH_DPP_SRC(v, 0x143, 0xC));
    return v;
}
// the value of the lane below (0 into lane 0)
__device__ __forceinline__ uint32_t wave_from_below(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138, 0xF, 0xF, true); // wave_shr:1
}

// Workgroup exclusive add-scan of one value per thread.  `lds` needs (threads/64)+1 words.
// Returns the exclusive prefix; *total receives the workgroup sum.
// (`tid`: the thread's index as the caller holds it -- a kernel that loops over work items and has made its index opaque
// per item passes that one, so that nothing here is hoisted out of its loop and kept alive across it)
__device__ __forceinline__ uint32_t block_excl_add_at(uint32_t v, uint32_t *lds, uint32_t *total, uint32_t tid)
{
    const int lane = tid & 63, wave = tid >> 6, nw = (blockDim.x + 63) >> 6;
    uint32_t inc = wave_incl_add(v, lane);
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    if (wave == 0) {
        uint32_t w = lane < nw ? lds[lane] : 0;
        uint32_t wi = wave_incl_add(w, lane);
        if (lane < nw) lds[lane] = wi - w;
        if (lane == nw - 1) lds[nw] = wi;
    }
    __syncthreads();
    uint32_t res = inc - v + lds[wave];
    *total = lds[nw];
    __syncthreads();
    return res;
}
__device__ __forceinline__ uint32_t block_excl_add(uint32_t v, uint32_t *lds, uint32_t *total)
{
    return block_excl_add_at(v, lds, total, threadIdx.x);
}

// Workgroup inclusive max-scan of one int per thread. `lds` needs (threads/64) ints.
__device__ __forceinline__ int block_incl_max(int v, int *lds)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    int inc = wave_incl_max(v, lane);
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    int carry = INT32_MIN;
    for (int w = 0; w < wave; w++) carry = max(carry, lds[w]);
    (void)nw;
    int res = max(inc, carry);
    __syncthreads();
    return res;
}

// Two inclusive max-scans at once (same barriers).  `lds` needs 2*(threads/64) ints.
__device__ __forceinline__ void block_incl_max2(int &a, int &b, int *lds)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    const int ia = wave_incl_max(a, lane), ib = wave_incl_max(b, lane);
    if (lane == 63) {
        lds[wave] = ia;
        lds[nw + wave] = ib;
    }
    __syncthreads();
    int ca = INT32_MIN, cb = INT32_MIN;
    for (int w = 0; w < wave; w++) {
        ca = max(ca, lds[w]);
        cb = max(cb, lds[nw + w]);
    }
    a = max(ia, ca);
    b = max(ib, cb);
    __syncthreads();
}

// Workgroup EXCLUSIVE suffix-min: result = min of v over all threads with a higher index (INT32_MAX for the
// last thread).  `lds` needs (threads/64) ints.
__device__ __forceinline__ int block_excl_min_rev(int v, int *lds)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    int inc = v; // inclusive suffix-min inside the wavefront
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_down(inc, d, 64);
        if (lane + d < 64) inc = min(inc, t);
    }
    if (lane == 0) lds[wave] = inc;
    __syncthreads();
    int carry = INT32_MAX;
    for (int w = wave + 1; w < nw; w++) carry = min(carry, lds[w]);
    int ex = __shfl_down(inc, 1, 64);
    if (lane == 63) ex = INT32_MAX;
    const int res = min(ex, carry);
    __syncthreads();
    return res;
}

// ---- stage entry points (host side, defined in the stage files) ---------------------------------
int bwt_run(bzh_ctx *ctx, uint32_t B, uint32_t nmax, uint64_t ntotal); // bwt.hip
int unbwt_run(bzh_ctx *ctx, uint32_t B, uint32_t nmax);               // bwt.hip: inverse transform, bt.bwt/ptr -> bt.unbwt_out
int unbwt_compare(bzh_ctx *ctx, uint32_t B, uint32_t nmax, unsigned long long *d_acc); // bwt.hip: bt.rle vs bt.unbwt_out
int mtf_run(bzh_ctx *ctx, uint32_t B, uint32_t nmax, uint64_t ntotal = 0); // mtf.hip (ntotal: statistics only)
int huff_prepare(bzh_ctx *ctx, uint32_t B, uint32_t mmax);            // huffman.hip: tables, header bits, bit totals
int huff_pack(bzh_ctx *ctx, uint32_t B, uint32_t mmax, uint8_t *d_out, uint64_t bit_base, bool gated = false); // huffman.hip
// (one batch, no host in between: zeroes the output words the batch's bits will occupy -- the first one may carry bits owed to
// it --, checks the capacity on the device and opens or shuts the gate of the pack kernels; hostrec[0] = bits, [1] = fits)
int huff_pack_gate(bzh_ctx *ctx, uint32_t B, uint8_t *d_out, uint64_t bit_base, uint64_t cap_words, uint32_t seed, bool has_seed,
                   uint64_t *hostrec, uint32_t tail_bits = 0);
int huff_frame_stream(bzh_ctx *ctx, uint32_t B, uint8_t *d_out); // huffman.hip: stream header + footer of a one-batch stream, on the device
int rle1_plan(bzh_ctx *ctx, const uint8_t *d_in, size_t n, bool with_crc = true, bool crc_async = false); // rle1.hip: tables + split from 0
int rle1_plan_tables(bzh_ctx *ctx, const uint8_t *d_in, size_t n, uint32_t extra_blocks = 0); // rle1.hip
int rle1_plan_many(bzh_ctx *ctx, const uint8_t *d_in, const size_t *lens, size_t count); // rle1.hip: plan of many inputs (bzh_plan_many_device)
// (one batch of a call over many inputs: stream layout, zeroing + capacity gate, pack, frames -- no host in between)
int huff_many_batch(bzh_ctx *ctx, const ManyBatch &mb, const uint32_t *d_binp, uint8_t *d_out, uint32_t mmax, const ManyOut &mo); // huffman.hip
int rle1_plan_split(bzh_ctx *ctx, size_t start, bool with_crc, size_t stop, bool crc_async = false); // rle1.hip
int rle1_plan_crc_join(bzh_ctx *ctx);                                             // rle1.hip: CRCs queued on the side stream -> plan_blocks
hipStream_t bzh_side_stream(bzh_ctx *ctx);                                        // api.hip: the context's second stream (created once; null: none to be had)
int rle1_plan_crc(bzh_ctx *ctx, size_t b0, size_t b1);               // rle1.hip: CRCs of plan blocks [b0, b1)
int rle1_emit(bzh_ctx *ctx, size_t b0, uint32_t B);                   // rle1.hip: fill bt.rle / bt.n / bt.desc
int crc_device(bzh_ctx *ctx, const uint8_t *d_in, size_t n, uint32_t *crc_out); // rle1.hip
// rle1.hip: CRCs of nb byte ranges of d_in (d_blocks[k].in_off / in_len, the longest maxlen bytes) into d_blocks[k].crc; no wait
int crc_blocks_device(bzh_ctx *ctx, const uint8_t *d_in, BlockDesc *d_blocks, uint32_t *d_acc, uint32_t nb, uint64_t maxlen);
struct CrcTables;                                                     // crc_gf.h
int crc_tables(bzh_ctx *ctx, const CrcTables **out);                  // rle1.hip: the context's device copy of the GF(2) tables
// decode.hip: every block / footer magic of d_in[0..n) as (bit position << 1 | kind), ascending; then the entropy stage and the
// chain walk over that list (the arena laid out for min(candidates, max_batch) blocks).  The back of the decoder -- inverse BWT,
// inverse RLE1, block CRCs -- is decode.hip's back_sizes / back_emit, which this and decode_range_run both call per batch.
int decode_scan_run(bzh_ctx *ctx, const uint8_t *d_in, size_t n, std::vector<uint64_t> &cands);
struct SyncBuild { // bzh_decode_index_sync*: the chain walk records a point every `interval` groups of every block on the chain
    uint32_t interval;
    std::vector<bzh_sync_point> pts;
};
struct RecBuild { // bzh_decode_index_records*: the index build also counts the delimiters of every block on the chain
    uint32_t delim;
    std::vector<uint64_t> cum; // [entries + 1] delimiters in front of every entry, and of the end
    bool last_is_delim;        // the last byte of the output is one
};
// A consumer of decoded windows (bzh_search*, bzh_grep*): the decoders expand WHOLE blocks, window after window, into a staging
// buffer that the sink owns, and hand every window over once all of its blocks have passed their CRCs.  This is all decode.hip
// knows of a search, a grep or a match (ScanSink below, and search.hip, grep.hip, match.hip: SearchSink, GrepSink, MatchSink).
struct WindowSink {
    const uint64_t front; // the decoders expand at *d_stage + front (whatever is carried between two windows lies in front of it)
    const uint32_t delim; // of the records, where the walk counts them (BackCount)
    // bytes in front of and behind the wanted range that what is looked for looks at (an automaton with assertions): a range decode
    // widens the decoded range by them, clipped to the output, and the sink still reports only what lies in the wanted range
    uint32_t look_behind = 0, look_ahead = 0;
    WindowSink(uint64_t front_, uint32_t delim_) : front(front_), delim(delim_) {}
    // the wanted range [lo, hi) of the output; the output offset of the first window's first byte, the delimiters in front of it
    virtual void begin(uint64_t lo, uint64_t hi, uint64_t out_start, uint64_t rec_start) = 0;
    // the staging for the next window of `bytes` decoded bytes: whole blocks, at least one, so a block above the target grows it
    virtual int room(bzh_ctx *ctx, uint64_t bytes, uint8_t **d_stage) = 0;
    // the window room() made room for has been expanded and verified
    virtual int window(bzh_ctx *ctx, uint64_t bytes) = 0;

protected:
    ~WindowSink() = default;
};
int decode_chain_run(bzh_ctx *ctx, const uint8_t *d_in, size_t n, uint8_t *d_out, size_t cap, size_t *out_len, size_t *consumed,
                     const std::vector<uint64_t> &cands, std::vector<bzh_index_entry> *index = nullptr, SyncBuild *sync = nullptr,
                     RecBuild *rec = nullptr, WindowSink *sink = nullptr);
// decode.hip: the two checks of an index and its sync points as a whole, then the blocks of a verified index that
// [off, off + len) touches, from d_in = the indexed input from byte in_byte_base on (windows and segments: decode_plan.h)
int decode_index_check(bzh_ctx *ctx, const bzh_index_entry *idx, size_t count); // BZH_E_ARG naming the entry that is ill formed
int decode_sync_check(bzh_ctx *ctx, const bzh_index_entry *idx, size_t count, const bzh_sync_point *pts, size_t npts); // same, the point
// (pts: sync points that have passed decode_sync_check; none: one wavefront a block.  count < 2^32, here and in the two below)
int decode_range_run(bzh_ctx *ctx, const uint8_t *d_in, size_t n, uint64_t in_byte_base, const bzh_index_entry *idx, size_t count,
                     uint64_t off, uint64_t len, uint8_t *d_out, size_t cap, size_t *out_len, const bzh_sync_point *pts = nullptr,
                     size_t npts = 0);
// decode.hip: the same over many ranges at once, every touched block decoded once.  touched / out_offs / out_total: what
// decode_plan.h's bzp_spans made of the ranges, out_total within the room at d_out
int decode_ranges_run(bzh_ctx *ctx, const uint8_t *d_in, size_t n, uint64_t in_byte_base, const bzh_index_entry *idx, size_t count,
                      const bzh_sync_point *pts, size_t npts, const bzh_range *ranges, size_t nranges, const size_t *out_offs,
                      const std::vector<uint32_t> &touched, uint8_t *d_out, uint64_t out_total);
// decode.hip: a read by record number over ascending ranges of records (the walk: decode_records_plan.h); the record table of raw bytes
int decode_records_run(bzh_ctx *ctx, const uint8_t *d_in, size_t n, uint64_t in_byte_base, const bzh_index_entry *idx, size_t count,
                       const bzh_sync_point *pts, size_t npts, const uint64_t *rec_cum, uint8_t delim, const bzh_range *ranges, size_t nranges,
                       const std::vector<uint32_t> &touched, uint8_t *d_out, size_t cap, size_t *out_offs, size_t *out_lens, size_t *out_total);
int count_records_run(bzh_ctx *ctx, const uint8_t *d_raw, size_t n, uint8_t delim, const bzh_index_entry *idx, size_t count, uint64_t *rec_cum,
                      uint64_t *nrecords);
// decode.hip: many inputs, one chain each, batches across them (the walk itself: decode_many_plan.h).  The slices have been checked.
int decode_many_run(bzh_ctx *ctx, const uint8_t *d_in, size_t n, const size_t *in_offs, const size_t *in_lens, size_t count, uint8_t *d_out,
                    size_t cap, size_t *out_offs, size_t *out_lens, int *status, size_t *consumed, const std::vector<uint64_t> &cands);
// decode.hip: every block magic judged on its own (the walk itself: decode_recover_plan.h); the block magics at `count` bit positions
int decode_recover_run(bzh_ctx *ctx, const uint8_t *d_in, size_t n, uint8_t *d_out, size_t cap, size_t *out_len,
                       std::vector<bzh_recover_entry> &entries, bzh_recover_stats &stats, const std::vector<uint64_t> &cands);
int decode_magic_run(bzh_ctx *ctx, const uint8_t *d_in, size_t n, const uint64_t *pos, size_t count, size_t *first_bad);
// decode.hip: the streaming decode (the walk and the feed loop: decode_stream_plan.h).  arena: api.hip's ensure_arena, called by
// every pass for the candidates it takes.  The pointers have been checked.
int dstream_begin(bzh_ctx *ctx);
int dstream_feed(bzh_ctx *ctx, int (*arena)(bzh_ctx *, uint32_t), const uint8_t *in, size_t n, int eof, size_t *in_used, uint8_t *out, size_t cap,
                 size_t *out_len, int *done);
size_t dstream_consumed(const bzh_ctx *ctx);
int dstream_stats(const bzh_ctx *ctx, bzh_dstream_stats *out);
void dstream_end(bzh_ctx *ctx);  // abandon: the buffers stay for the next begin
void dstream_free(bzh_ctx *ctx); // bzh_destroy
// decode.hip: the blocks that output [off, off + len) of an indexed input touches, window by window into a sink, which applies the
// range (rec_cum: the record table, for a sink that numbers records; null: none)
int decode_range_sink_run(bzh_ctx *ctx, const uint8_t *d_in, size_t n, uint64_t in_byte_base, const bzh_index_entry *idx, size_t count,
                          const bzh_sync_point *pts, size_t npts, const uint64_t *rec_cum, uint64_t off, uint64_t len, WindowSink &sink);
// search.hip: what the two sinks share on the host.  scan_room: ctx->search_ws grown to a window of `bytes` behind a carry of `carry`
// bytes, which is copied from ctx->scan_carry in front of the new bytes; *front = their staging position, *d_stage as
// WindowSink::room's.  scan_tiles: the tiles of a window of n bytes, counted into the call's statistics.
int scan_room(bzh_ctx *ctx, const char *what, uint64_t carry, uint64_t bytes, uint64_t *staging_peak, uint8_t **d_stage, uint64_t *front);
int scan_tiles(bzh_ctx *ctx, const char *who, uint64_t n, uint64_t *windows, uint64_t *tiles_sum, uint32_t *tiles);
// patset.hip: a compiled set of patterns (patset_plan.h), resident on its device in one allocation of its own -- it belongs to no
// context.  (As the kernels take it: matcher_pick.h)
struct bzh_patset {
    int device;
    bzh_patset_info info;
    bool regex = false;    // regex.hip made it: the table is a DFA's (regex_plan.h), the matcher BzrMatcher<.., false>
    bzh_regex_info rinfo{};
    uint32_t nterm = 0;    // of a regex: the terminal rows 1 .. nterm (a set's: info.distinct)
    bzh_regex_look look{}; // of a regex with assertions: what it looks at (both 0: none; else the matcher is BzrMatcher<.., true>)
    uint32_t ctx_row = 0;  // ... the start row of context c in bits [8 c, 8 c + 8)
    uint8_t *d_mem; // cls[256], first[256 * contexts], pat_no[distinct], table[states * classes]; with assertions pat_ctx[4 nterm], acc_mask[nterm]
    const uint8_t *d_cls;
    const uint16_t *d_first, *d_table;
    const uint32_t *d_pat_no;
    const uint32_t *d_pat_ctx = nullptr;
    const uint8_t *d_acc_mask = nullptr;
    bool looks() const { return look.look_behind || look.look_ahead; }
};
// What a search, a grep or a match looks for: a byte string, or a compiled set (bzh_*_patset*).
struct ScanWhat {
    const uint8_t *pat;
    size_t plen;
    const bzh_patset *set;
    bool is_set;
    bool given() const { return is_set ? set != nullptr : pat != nullptr; }
};
// What a call of bzh_search* / bzh_grep* / bzh_match* was given beside its input, as the caller wrote it: nothing of it has been
// checked.  out / cap: where the bytes go (device; a search writes none), ent / max: the entries or the hits (host).
struct ScanArgs {
    ScanWhat what;
    unsigned flags;
    void *out;
    size_t cap;
    void *ent;
    size_t max;
};
// The sink of one such call, as api.hip's routes know it: a WindowSink for the decoders, and beside the windows what every route
// does once a call -- the one window of decoded bytes that already lie in HBM, what is left behind the last window, and the
// answer.  The constructor only keeps the arguments; arm() makes the walk of them once the route has checked them.
struct ScanSink : WindowSink {
    ScanArgs args;
    ScanSink(const ScanWhat &q, unsigned flags, uint8_t delim_, void *out, size_t cap, void *ent, size_t max)
        : WindowSink(BZF_FRONT, delim_), args{q, flags, out, cap, ent, max} {}
    virtual void arm(const bzh_ctx *ctx) = 0;
    // decoded bytes that already lie in HBM: one window, no staging, no carry
    virtual int raw(bzh_ctx *ctx, const uint8_t *d_raw, size_t n) = 0;
    // behind the last window: what was held back is processed where it lies, in the carry
    virtual int finish(bzh_ctx *ctx) = 0;
    // behind the last wait: the counts to the caller; BZH_E_CAP, with its text, where a room was too small
    virtual int report(bzh_ctx *ctx, size_t *count, uint64_t *out_total) = 0;

protected:
    ~ScanSink() = default;
};
// search.hip: the search over decoded bytes in HBM.  A sink is what is looked for, where the hits go, and the walk over its windows
// (search_plan.h): room() puts the carry in front of the window, window() runs the two passes and keeps the window's tail;
// finish() of a set search: the starts held back.
struct SearchSink final : ScanSink {
    BzfPattern pat{};
    const bzh_patset *set = nullptr; // what is looked for instead of pat: hits are bzh_set_hit, the windows BzmSetWalk::window_set's
    bool records = false;
    void *hits = nullptr; // host: bzh_hit, or bzh_set_hit
    uint64_t max = 0;
    BzmSetWalk walk; // (a single pattern keeps to BzfWalk's part of it)
    SearchSink(const ScanWhat &q, unsigned flags, uint8_t delim_, void *hits_, size_t max_) : ScanSink(q, flags, delim_, nullptr, 0, hits_, max_) {}
    void arm(const bzh_ctx *) override
    {
        const ScanWhat &q = args.what;
        if (q.is_set) set = q.set, look_behind = set->look.look_behind, look_ahead = set->look.look_ahead;
        else pat = bzf_pattern(q.pat, (uint32_t)q.plen, delim);
        records = (args.flags & BZH_SEARCH_RECORDS) != 0, hits = args.ent, max = args.max;
    }
    bool looks() const { return set && set->looks(); }
    uint32_t plen() const { return set ? set->info.max_len : pat.plen; } // (of a set: its longest pattern's)
    size_t hit_size() const { return set ? sizeof(bzh_set_hit) : sizeof(bzh_hit); }
    void begin(uint64_t lo, uint64_t hi, uint64_t out_start, uint64_t rec_start) override
    {
        walk.begin(plen(), front, max, lo, hi, out_start, rec_start);
        walk.begin_look(look_behind, look_ahead);
    }
    int room(bzh_ctx *ctx, uint64_t bytes, uint8_t **d_stage) override;
    int window(bzh_ctx *ctx, uint64_t bytes) override;
    int raw(bzh_ctx *ctx, const uint8_t *d_raw, size_t n) override;
    int finish(bzh_ctx *ctx) override;
    int report(bzh_ctx *ctx, size_t *nhits, uint64_t *) override;
};
// grep.hip: the selected records of decoded bytes in HBM, compacted into d_out.  A sink is what is looked for, where bytes and
// entries go, and the walk over its windows (grep_plan.h): as the search's, with the whole open record carried (begin() has nothing
// to say: a grep takes the whole output).  finish(): the bytes held back and the open tail, behind the last window.
struct GrepSink final : ScanSink {
    BzfPattern pat{};
    const bzh_patset *set = nullptr; // what is looked for instead of pat; the walk keeps its rule with plen = the longest pattern's
    uint8_t *d_out = nullptr;      // device (null: not asked for)
    bzh_grep_entry *ent = nullptr; // host (null: not asked for)
    BzgWalk walk;
    BzcWalk cwalk;       // the walk instead of it when context records are asked for (grep_ctx_plan.h)
    bool ctx_on = false;
    uint64_t at = 0;               // staging position of the window's first new byte
    const uint8_t *tail = nullptr; // device: where the carry lies
    BzgEntry tail_ent{};           // finish(): the open tail's entry, which report() stores at ent[sel - 1] behind the last wait ...
    bool tail_ent_due = false;     // ... where it is a selected record with room for its entry
    GrepSink(const ScanWhat &q, unsigned flags, uint8_t delim_, void *d_out_, size_t cap, bzh_grep_entry *ent_, size_t max)
        : ScanSink(q, flags, delim_, d_out_, cap, ent_, max) {}
    // the context's bzh_grep_set_context as the call finds it
    void arm(const bzh_ctx *ctx) override
    {
        const ScanWhat &q = args.what;
        const bool invert = (args.flags & BZH_GREP_INVERT) != 0;
        d_out = (uint8_t *)args.out, ent = (bzh_grep_entry *)args.ent;
        if (q.is_set) {
            set = q.set;
            walk.begin(set->info.max_len + set->look.look_ahead, invert, d_out != nullptr, args.cap, ent != nullptr, args.max); // (the hold-back grows by the byte behind a match)
        } else {
            pat = bzf_pattern(q.pat, (uint32_t)q.plen, delim);
            walk.begin((uint32_t)q.plen, invert, d_out != nullptr, args.cap, ent != nullptr, args.max);
        }
        set_context(ctx->grep_before, ctx->grep_after);
    }
    // 0, 0 leaves the plain walk and its kernels
    void set_context(uint32_t before, uint32_t after)
    {
        ctx_on = before || after;
        if (ctx_on) cwalk.begin(walk.plen, walk.invert != 0, before, after, walk.want_out, walk.cap, walk.want_ent, walk.max);
    }
    uint64_t carry() const { return ctx_on ? cwalk.carry : walk.carry; }
    uint64_t sel() const { return ctx_on ? cwalk.sel : walk.sel; }
    uint64_t out_bytes() const { return ctx_on ? cwalk.out_bytes : walk.out_bytes; }
    bool overflow() const { return ctx_on ? cwalk.overflow() : walk.overflow(); }
    void begin(uint64_t, uint64_t, uint64_t, uint64_t) override {}
    int room(bzh_ctx *ctx, uint64_t bytes, uint8_t **d_stage) override;
    int window(bzh_ctx *ctx, uint64_t bytes) override;
    int raw(bzh_ctx *ctx, const uint8_t *d_raw, size_t n) override;
    // grep_many.hip: many texts that lie in one buffer in HBM, with walls between them (the tables: grep_many_plan.h) -- one
    // segmented pass, no staging, no carry, no tail: finish() finds nothing left.  seg_totals: [texts][BZGM_TOTALS], on the host
    // behind the pass's wait
    int raw_many(bzh_ctx *ctx, const uint8_t *d_raw, const struct BzgmPlan &plan, uint64_t *seg_totals);
    int finish(bzh_ctx *ctx) override;
    int report(bzh_ctx *ctx, size_t *nrecs, uint64_t *out_total) override;
};
// match.hip: the selected matches of decoded bytes in HBM, compacted into d_out.  A sink is what is looked for, where bytes and
// entries go, and the walk over its windows (match_plan.h): a set search's hold-back and the cursor.  finish(): the starts held
// back, behind the last window.
struct MatchSink final : ScanSink {
    BzfPattern pat{};
    const bzh_patset *set = nullptr; // what is looked for instead of pat
    bool records = false;
    uint8_t *d_out = nullptr;       // device (null: not asked for)
    bzh_match_entry *ent = nullptr; // host (null: not asked for)
    MtWalk walk;
    uint64_t at = 0; // staging position of the window's first new byte
    MatchSink(const ScanWhat &q, unsigned flags, uint8_t delim_, void *d_out_, size_t cap, bzh_match_entry *ent_, size_t max)
        : ScanSink(q, flags, delim_, d_out_, cap, ent_, max) {}
    void arm(const bzh_ctx *) override
    {
        const ScanWhat &q = args.what;
        records = (args.flags & BZH_MATCH_RECORDS) != 0, d_out = (uint8_t *)args.out, ent = (bzh_match_entry *)args.ent;
        if (q.is_set) {
            set = q.set, look_behind = set->look.look_behind, look_ahead = set->look.look_ahead;
            walk.begin(set->info.max_len, look_behind, look_ahead, true, d_out != nullptr, args.cap, ent != nullptr, args.max);
        } else {
            pat = bzf_pattern(q.pat, (uint32_t)q.plen, delim);
            walk.begin((uint32_t)q.plen, 0, 0, false, d_out != nullptr, args.cap, ent != nullptr, args.max);
        }
    }
    void begin(uint64_t, uint64_t, uint64_t, uint64_t) override {} // (the whole output, from offset 0)
    int room(bzh_ctx *ctx, uint64_t bytes, uint8_t **d_stage) override;
    int window(bzh_ctx *ctx, uint64_t bytes) override;
    int raw(bzh_ctx *ctx, const uint8_t *d_raw, size_t n) override;
    int finish(bzh_ctx *ctx) override;
    int report(bzh_ctx *ctx, size_t *nmatches, uint64_t *out_total) override;
};
// recover.hip: the bits of the kept blocks, end to end from bit 32 of d_out, in one launch (the per-word rule: recover_gather.h)
struct BzrDesc;
int recover_gather_run(bzh_ctx *ctx, const uint8_t *d_in, size_t n, const std::vector<BzrDesc> &descs, uint64_t body, uint32_t *d_out);
// unbwt_small.hip: the inverse BWT in LDS of the K listed batch slots, blocks of at most bzh_decode_many_small_max() bytes each
// (bt.bwt / bt.n / bt.ptr -> bt.unbwt_out, as unbwt_run); its switch; the first four bytes of many slices in one launch
int unbwt_small_run(bzh_ctx *ctx, const uint32_t *d_slots, uint32_t K);
bool unbwt_small_enabled();
int many_heads_run(bzh_ctx *ctx, const uint8_t *d_in, const uint64_t *d_offs, const uint64_t *d_lens, uint32_t count, uint32_t *d_heads);

// sync_emit.hip: the index of the stream being encoded (bzh_encode_index*).  encode_range hands every batch over once its bits
// are packed and before its arena is reused: the entries of its blocks, and a sync point every `interval` groups (0: none)
struct EncIndex {
    uint32_t interval;
    std::vector<bzh_index_entry> entries;
    std::vector<bzh_sync_point> pts;
};
int sync_emit_batch(bzh_ctx *ctx, uint32_t B, size_t k0, uint64_t bit_base, EncIndex &ix);
