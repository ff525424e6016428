// grep.hip -- the records of decoded bytes in HBM that hold a byte string, compacted into the caller's buffer (bzh_grep*): the two
// passes over the tiles of a window, the scan between them, and the grep as a ScanSink (common.h): its staging room (search.hip's
// scan_room), the carry between two windows, what is left behind the last one, and the answer.  The windows: grep_plan.h; the tile front: search_core.h; what
// one thread, one tile and the scan do behind it: grep_core.h.  The text never leaves the device: what comes back is five words a
// window, and the selected records.
#include "common.h"
#include "grep_core.h"
#include "grep_ctx_core.h"
#include "matcher_pick.h"

static_assert(sizeof(bzh_grep_entry) == 32 && sizeof(BzgEntry) == sizeof(bzh_grep_entry), "an entry is four words");
static_assert(sizeof(BzgTile) == 32 && sizeof(BzgBase) == 24, "the tile tables");

struct GfArgs {
    const uint8_t *d; // 16-byte aligned
    BzgWindow win;
    BzgTile *tile;       // [tiles] pass one writes, the scan completes, pass two reads
    const BzgBase *base; // [tiles] the scan: what lies in front of every tile
    uint8_t *out;        // the caller's bytes (null: only entries are asked for); 4-byte aligned
    BzgEntry *ent;       // the window's entries [0, selected) (null: only bytes are asked for)
};

// One workgroup a tile of 4,096 positions, 16 a thread; the tile, the halo behind it and what the matcher M keeps beside them are
// staged in LDS by the front it shares with search_tiles (search_core.h; the matchers: patset_core.h).  A set bounds its matches by
// the text's end itself, so every processed position is one of its starts.  GATHER false: the tile's record (BzgTile), one plain store -- no atomics; grep_scan joins the tiles.  GATHER true,
// in tiles that hold selected bytes: the same masks again, the selection of every byte, the selected ones compacted in LDS and
// written to out[out_base + base.out ..) -- bytes of this tile only, to addresses no other workgroup writes: words inside the run,
// single bytes at its two ends -- and an entry from every thread that holds a selected record's delimiter.
template <bool GATHER, class M>
__global__ void __launch_bounds__(BZF_THREADS) grep_tiles(GfArgs a, M m)
{
    __shared__ __attribute__((aligned(16))) uint8_t tile[BZF_TILE + BZF_MAX_PATTERN];
    __shared__ typename M::Shared msh;
    __shared__ BzgShared sh;
    const uint32_t tid = threadIdx.x;
    BzgTile x{};
    BzgBase base{};
    if (GATHER) {
        x = a.tile[blockIdx.x];
        if (x.bytes == 0) return; // (the same for every thread; a selected record's delimiter is one of its bytes)
        base = a.base[blockIdx.x];
    }
    const uint64_t t0 = (uint64_t)blockIdx.x * BZF_TILE, p0 = t0 + tid * BZF_ITEMS;
    const BzfVec own = m.stage(a.d, a.win.n, t0, tid, tile, msh);
    __syncthreads();
    BzgThread t;
    const uint32_t starts = M::BY_LIM ? bzf_range_mask16(p0, a.win.p_lo, a.win.p_hi) : bzg_starts(a.win, p0);
    bzg_masks(t, a.win, p0, own, m.delim(), m.match16(own, tid, p0, tile, msh, starts));
    bzg_local(t, a.win.invert);
    bzg_count_p0(sh, tid, t);
    __syncthreads();
    for (uint32_t k = 0; k < 8; k++) {
        bzg_step_f(sh, tid, k);
        __syncthreads();
    }
    if (!GATHER) {
        bzg_count_p1(sh, tid, t, a.win.invert);
        __syncthreads();
        for (uint32_t k = 0; k < 8; k++) {
            bzg_step_s(sh, tid, k);
            __syncthreads();
        }
        if (tid == 0) {
            BzgTile o;
            bzg_count_p2(sh, o);
            a.tile[blockIdx.x] = o;
        }
        return;
    }
    bool sel_first;
    bzg_gather_p1(sh, tid, t, x, a.win.invert, &sel_first);
    __syncthreads();
    for (uint32_t k = 0; k < 8; k++) {
        bzg_step_b(sh, tid, k);
        __syncthreads();
    }
    uint32_t sm, sdm;
    bzg_gather_p2(sh, tid, t, x, sel_first, &sm, &sdm);
    __syncthreads();
    for (uint32_t k = 0; k < 8; k++) {
        bzg_step_s(sh, tid, k);
        __syncthreads();
    }
    uint8_t *dst = a.out ? a.out + a.win.out_base + base.out : nullptr;
    const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3u);
    bzg_gather_p3(sh, tid, blockIdx.x, t, x, base, a.win, tile + tid * BZF_ITEMS, sm, sdm, shift, dst != nullptr, a.ent);
    if (!dst) return;
    __syncthreads();
    bzg_gather_p4(sh, tid, dst, shift, x.bytes);
}

// The tiles of a window joined in one workgroup, every thread a run of consecutive tiles: forward, which record enters every tile
// and whether it holds a match; backward, whether the record that leaves it is selected; then the sums in front of every tile.
__global__ void __launch_bounds__(BZF_THREADS) grep_scan(BzgTile *tile, uint32_t tiles, BzgBase *base, BzgWindow w, uint64_t *totals)
{
    __shared__ BzgScanShared sh;
    const uint32_t tid = threadIdx.x;
    bzg_scan_a(sh, tid, tile, tiles);
    __syncthreads();
    if (tid == 0) bzg_scan_b(sh, w, totals);
    __syncthreads();
    bzg_scan_c(sh, tid, tile, tiles, w);
    __syncthreads();
    if (tid == 0) bzg_scan_d(sh);
    __syncthreads();
    bzg_scan_e(sh, tid, tile, tiles, w);
    __syncthreads();
    if (tid == 0) bzg_scan_f(sh, totals);
    __syncthreads();
    bzg_scan_g(sh, tid, tile, tiles, base);
}

// ---- context records (bzh_grep_set_context; the phases: grep_ctx_core.h) ------------------------------------------------------------
static_assert(sizeof(BzcTile) == 48 && sizeof(BzcCount) == 16, "the context grep's tile tables");

struct GcArgs {
    const uint8_t *d; // 16-byte aligned
    BzcWindow win;
    BzcTile *tile;    // [tiles] pass one writes, scan one completes
    BzcCount *cnt;    // [tiles] pass two
    BzgBase *base;    // [tiles] del: scan one; out, sel: scan two
    uint16_t *hits;   // [tiles * 256] every thread's hit starts: pass one writes, the later passes read
    uint64_t *totals; // [BZC_TOTALS]
    uint8_t *out;
    BzgEntry *ent;
};

// Pass one: grep_tiles' front with the matcher M, every thread's hit starts into the table, the tile's record.
template <class M>
__global__ void __launch_bounds__(BZF_THREADS) grep_ctx_tiles(GcArgs a, M m)
{
    __shared__ __attribute__((aligned(16))) uint8_t tile[BZF_TILE + BZF_MAX_PATTERN];
    __shared__ typename M::Shared msh;
    __shared__ BzcShared sh;
    const uint32_t tid = threadIdx.x;
    const uint64_t t0 = (uint64_t)blockIdx.x * BZF_TILE, p0 = t0 + tid * BZF_ITEMS;
    const BzfVec own = m.stage(a.d, a.win.w.n, t0, tid, tile, msh);
    __syncthreads();
    BzgThread t;
    const uint32_t starts = M::BY_LIM ? bzf_range_mask16(p0, a.win.w.p_lo, a.win.w.p_hi) : bzg_starts(a.win.w, p0);
    const uint32_t hm = m.match16(own, tid, p0, tile, msh, starts);
    a.hits[(size_t)blockIdx.x * BZF_THREADS + tid] = (uint16_t)hm;
    bzc_masks(t, a.win, p0, own, m.delim(), hm);
    bzg_count_p0(sh.g, tid, t);
    __syncthreads();
    for (uint32_t k = 0; k < 8; k++) {
        bzg_step_f(sh.g, tid, k);
        __syncthreads();
    }
    bzc_count_p1(sh, tid, t, a.win, p0);
    __syncthreads();
    for (uint32_t k = 0; k < 8; k++) {
        bzc_step(sh, tid, k);
        bzg_step_s(sh.g, tid, k);
        __syncthreads();
    }
    if (tid == 0) {
        BzcTile o;
        bzc_count_p2(sh, o);
        a.tile[blockIdx.x] = o;
    }
}

// Scan one, one workgroup: the hit state, the open record and the distance to the last primary at every tile's entry, the
// distance to the next primary at its exit; the window's tail and the records that stay pending.
__global__ void __launch_bounds__(BZF_THREADS) grep_ctx_scan(BzcTile *tile, uint32_t tiles, BzgBase *base, BzcWindow w, uint64_t *totals)
{
    __shared__ BzcScanShared sh;
    const uint32_t tid = threadIdx.x;
    bzc_scan_a(sh, tid, tile, tiles, w);
    __syncthreads();
    if (tid == 0) bzc_scan_b(sh, w, totals);
    __syncthreads();
    bzc_scan_c(sh, tid, tile, tiles, w, base);
    __syncthreads();
    if (tid == 0) bzc_scan_d(sh, w, totals);
    __syncthreads();
    bzc_scan_e(sh, tid, tile, tiles, w);
}

// Passes two and three: the selection of every record of the tile from the hit table and the distances at the tile's edges.
// GATHER false: the tile's counts; the one thread that holds the first pending record's start stores it.  GATHER true, in
// tiles that hold selected bytes: compaction and entries as grep_tiles', bit 63 of len on context records.
template <bool GATHER>
__global__ void __launch_bounds__(BZF_THREADS) grep_ctx_select(GcArgs a, uint32_t delim)
{
    __shared__ __attribute__((aligned(16))) uint8_t tile[GATHER ? BZF_TILE : 16]; // (the gather compacts from it)
    __shared__ BzcShared sh;
    const uint32_t tid = threadIdx.x;
    BzcCount c{};
    if (GATHER) {
        c = a.cnt[blockIdx.x];
        if (c.bytes == 0) return; // (the same for every thread)
    }
    const BzcTile x = a.tile[blockIdx.x];
    const BzgBase base = a.base[blockIdx.x];
    const uint64_t t0 = (uint64_t)blockIdx.x * BZF_TILE, p0 = t0 + tid * BZF_ITEMS;
    const BzfVec own = bzf_load16(a.d, a.win.w.n, p0);
    if (GATHER) *reinterpret_cast<BzfVec *>(tile + tid * BZF_ITEMS) = own; // (read back by this thread only)
    BzgThread t;
    bzc_masks(t, a.win, p0, own, delim, a.hits[(size_t)blockIdx.x * BZF_THREADS + tid]);
    bzg_count_p0(sh.g, tid, t);
    __syncthreads();
    for (uint32_t k = 0; k < 8; k++) {
        bzg_step_f(sh.g, tid, k);
        __syncthreads();
    }
    const uint32_t pm = bzc_sel_p1(sh, tid, t, x, a.win, p0);
    __syncthreads();
    for (uint32_t k = 0; k < 8; k++) {
        bzc_step(sh, tid, k);
        __syncthreads();
    }
    const bool first_rec = a.win.w.rec_base == 0 && base.del == 0;
    uint64_t pend = ~0ull;
    const uint64_t find = GATHER ? ~0ull : a.totals[BZC_T_PEND_FIND], behind = GATHER ? 0 : a.totals[BZG_T_DEL] - base.del - x.nd;
    const BzcSel r = bzc_sel_p2(sh, tid, t, pm, x, a.win, first_rec, p0, find, behind, &pend);
    if (!GATHER) {
        if (pend != ~0ull) a.totals[BZC_T_PEND_START] = pend; // (one thread of the window)
        bzc_count2_p3(sh, tid, r);
        __syncthreads();
        for (uint32_t k = 0; k < 8; k++) {
            bzg_step_s(sh.g, tid, k);
            __syncthreads();
        }
        if (tid == 0) {
            BzcCount o;
            bzc_count2_p4(sh, o);
            a.cnt[blockIdx.x] = o;
        }
        return;
    }
    bzc_gather_p3(sh, tid, t, r);
    __syncthreads();
    for (uint32_t k = 0; k < 8; k++) {
        bzg_step_s(sh.g, tid, k);
        __syncthreads();
    }
    uint8_t *dst = a.out ? a.out + a.win.w.out_base + base.out : nullptr;
    const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3u);
    BzgTile xg{};
    xg.open_start = x.open_start;
    bzg_gather_p3(sh.g, tid, blockIdx.x, t, xg, base, a.win.w, tile + tid * BZF_ITEMS, r.sm, r.sdm, shift, dst != nullptr, a.ent);
    bzc_gather_mark(sh, tid, base, r, a.ent);
    if (!dst) return;
    __syncthreads();
    bzg_gather_p4(sh.g, tid, dst, shift, c.bytes);
}

// Scan two, one workgroup: the sums in front of every tile, the window's totals.
__global__ void __launch_bounds__(BZF_THREADS) grep_ctx_sum(const BzcCount *cnt, uint32_t tiles, BzgBase *base, uint64_t *totals)
{
    __shared__ BzcSumShared sh;
    const uint32_t tid = threadIdx.x;
    bzc_sum_a(sh, tid, cnt, tiles);
    __syncthreads();
    if (tid == 0) bzc_sum_b(sh, totals);
    __syncthreads();
    bzc_sum_c(sh, tid, cnt, tiles, base);
}

// ---- host side ---------------------------------------------------------------------------------------------------
// The passes over the window w of d (16-byte aligned; w.n bytes lie there, and the aligned word that holds the last of them).  One
// wait, for the window's totals; bytes and entries follow the stream and are there after the call's last wait.
static int grep_window_run(bzh_ctx *ctx, GrepSink &g, const uint8_t *d, const BzgWindow &w, uint64_t bytes)
{
    hipStream_t st = ctx->stream;
    bzh_grep_stats &gs = ctx->gstats;
    // the text begins at a record start: the text's edge at output offset 0, else the delimiter stands in front of it
    const BzfPick pick{w.n, w.n, w.t_lo, w.off_base + w.t_lo == 0 ? (uint32_t)BZR_LOOK_EDGE : bzr_ctx(g.delim)};
    uint32_t tiles;
    BZH_TRY(scan_tiles(ctx, "grep", w.n, &gs.windows, &gs.tiles, &tiles));
    uint64_t totals[BZG_TOTALS] = {0, 0, 0, w.t_lo, w.open_hit};
    if (tiles && w.p_hi > w.p_lo) {
        BzgTile *tile = nullptr;
        BzgBase *base = nullptr;
        uint64_t *d_tot = nullptr;
        BZH_TRY(reserve_cut(ctx, ctx->grep_tab, "the grep's tile tables", grow_mib,
                            [&](Carver &c) { c.put(tile, tiles), c.put(base, tiles), c.put(d_tot, BZG_TOTALS); }));
        GfArgs a{d, w, tile, base, nullptr, nullptr};
        pick_matcher(g.pat, g.set, g.delim, pick, [&](const auto &m) { grep_tiles<false><<<dim3(tiles), BZF_THREADS, 0, st>>>(a, m); });
        grep_scan<<<dim3(1), BZF_THREADS, 0, st>>>(tile, tiles, base, w, d_tot);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(totals, d_tot, sizeof totals, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, bzh_stream_wait(st));
        if (g.walk.gather(totals)) {
            a.out = g.walk.want_out ? g.d_out : nullptr;
            if (g.walk.want_ent) {
                BZH_TRY(ctx->grep_ent.reserve(ctx, (size_t)totals[BZG_T_SEL] * sizeof(BzgEntry), "the grep's entries", grow_mib));
                a.ent = ctx->grep_ent.as<BzgEntry>();
            }
            pick_matcher(g.pat, g.set, g.delim, pick, [&](const auto &m) { grep_tiles<true><<<dim3(tiles), BZF_THREADS, 0, st>>>(a, m); });
            HIP_TRY(ctx, hipGetLastError());
            if (a.ent)
                HIP_TRY(ctx, hipMemcpyAsync(g.ent + w.sel_base, a.ent, (size_t)totals[BZG_T_SEL] * sizeof(BzgEntry), hipMemcpyDeviceToHost, st));
        }
    }
    g.walk.advance(w, bytes, totals);
    g.tail = d + totals[BZG_T_TAIL_START];
    gs.carry_peak = g.walk.carry_peak;
    return BZH_OK;
}

// The same with context records: three passes and two scans over the window (grep_ctx_core.h), still one wait.
static int grep_ctx_window_run(bzh_ctx *ctx, GrepSink &g, const uint8_t *d, const BzcWindow &w, uint64_t bytes)
{
    hipStream_t st = ctx->stream;
    bzh_grep_stats &gs = ctx->gstats;
    const BzfPick pick{w.w.n, w.w.n, w.w.t_lo, w.w.off_base + w.w.t_lo == 0 ? (uint32_t)BZR_LOOK_EDGE : bzr_ctx(g.delim)};
    uint32_t tiles;
    BZH_TRY(scan_tiles(ctx, "grep", w.w.n, &gs.windows, &gs.tiles, &tiles));
    uint64_t totals[BZC_TOTALS];
    g.cwalk.totals_idle(w, totals);
    if (g.cwalk.runs(w)) {
        GcArgs a{d, w, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        BZH_TRY(reserve_cut(ctx, ctx->grep_tab, "the grep's tile tables", grow_mib, [&](Carver &c) {
            c.put(a.tile, tiles), c.put(a.base, tiles), c.put(a.totals, BZC_TOTALS), c.put(a.cnt, tiles), c.put(a.hits, (size_t)tiles * BZF_THREADS);
        }));
        pick_matcher(g.pat, g.set, g.delim, pick, [&](const auto &m) { grep_ctx_tiles<<<dim3(tiles), BZF_THREADS, 0, st>>>(a, m); });
        grep_ctx_scan<<<dim3(1), BZF_THREADS, 0, st>>>(a.tile, tiles, a.base, w, a.totals);
        grep_ctx_select<false><<<dim3(tiles), BZF_THREADS, 0, st>>>(a, g.delim);
        grep_ctx_sum<<<dim3(1), BZF_THREADS, 0, st>>>(a.cnt, tiles, a.base, a.totals);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(totals, a.totals, sizeof totals, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, bzh_stream_wait(st));
        if (g.cwalk.gather(totals)) {
            a.out = g.cwalk.want_out ? g.d_out : nullptr;
            if (g.cwalk.want_ent) {
                BZH_TRY(ctx->grep_ent.reserve(ctx, (size_t)totals[BZG_T_SEL] * sizeof(BzgEntry), "the grep's entries", grow_mib));
                a.ent = ctx->grep_ent.as<BzgEntry>();
            }
            grep_ctx_select<true><<<dim3(tiles), BZF_THREADS, 0, st>>>(a, g.delim);
            HIP_TRY(ctx, hipGetLastError());
            if (a.ent)
                HIP_TRY(ctx, hipMemcpyAsync(g.ent + w.w.sel_base, a.ent, (size_t)totals[BZG_T_SEL] * sizeof(BzgEntry), hipMemcpyDeviceToHost, st));
        }
    }
    g.cwalk.advance(w, bytes, totals);
    g.tail = d + totals[BZC_T_PEND_START];
    gs.carry_peak = g.cwalk.carry_peak;
    return BZH_OK;
}

int GrepSink::room(bzh_ctx *ctx, uint64_t bytes, uint8_t **d_stage)
{
    return scan_room(ctx, "the grep's staging", carry(), bytes, &ctx->gstats.staging_peak, d_stage, &at);
}

// The passes, then everything behind the last delimiter they processed is kept as the carry.  (The copy is queued behind the
// window's wait -- where the tail starts is one of its totals -- and reserve() waits for the stream before it frees, so the staging
// buffer outlives it.)
int GrepSink::window(bzh_ctx *ctx, uint64_t bytes)
{
    if (ctx_on) BZH_TRY(grep_ctx_window_run(ctx, *this, ctx->search_ws.p, cwalk.window(at, bytes, false), bytes));
    else BZH_TRY(grep_window_run(ctx, *this, ctx->search_ws.p, walk.window(at, bytes, false), bytes));
    const uint64_t keep = carry();
    BZH_TRY(ctx->scan_carry.reserve(ctx, (size_t)keep + 16, "the grep's carry", grow_mib));
    if (keep) HIP_TRY(ctx, hipMemcpyAsync(ctx->scan_carry, tail, (size_t)keep, hipMemcpyDeviceToDevice, ctx->stream));
    tail = ctx->scan_carry;
    return BZH_OK;
}

// Decoded bytes that already lie in HBM: one window, no staging, no carry.
int GrepSink::raw(bzh_ctx *ctx, const uint8_t *d_raw, size_t n)
{
    if (ctx_on) return grep_ctx_window_run(ctx, *this, d_raw, cwalk.window(0, n, true), n);
    return grep_window_run(ctx, *this, d_raw, walk.window(0, n, true), n);
}

// Behind the last window: the bytes held back are processed where they lie, in the carry; then the open tail, if it is a selected
// record, goes out in one copy.  tail_ent_due: report() stores the tail's entry at ent[sel - 1] behind the call's last wait.
int GrepSink::finish(bzh_ctx *ctx)
{
    tail_ent_due = false;
    bzh_grep_stats &gs = ctx->gstats;
    if (ctx_on) { // the finishing window also where records are pending: a primary tail selects them
        BzcWalk &cw = cwalk;
        if (cw.held || cw.npend) BZH_TRY(grep_ctx_window_run(ctx, *this, ctx->scan_carry, cw.window(cw.carry, 0, true), 0));
        bool copy = false;
        cw.tail_rooms(&copy, &tail_ent_due);
        tail_ent = cw.tail_entry();
        if (copy) HIP_TRY(ctx, hipMemcpyAsync(d_out + cw.out_bytes, tail, (size_t)cw.carry, hipMemcpyDeviceToDevice, ctx->stream));
        cw.tail_done();
        gs.records = cw.nrecords(), gs.selected = cw.sel, gs.out_bytes = cw.out_bytes;
        ctx->gcstats = bzh_grep_context_stats{cw.matched, cw.context, cw.groups, cw.pending_peak};
        return BZH_OK;
    }
    if (walk.held) BZH_TRY(grep_window_run(ctx, *this, ctx->scan_carry, walk.window(walk.carry, 0, true), 0));
    bool copy = false;
    walk.tail_rooms(&copy, &tail_ent_due);
    tail_ent = walk.tail_entry();
    if (copy) HIP_TRY(ctx, hipMemcpyAsync(d_out + walk.out_bytes, tail, (size_t)walk.carry, hipMemcpyDeviceToDevice, ctx->stream));
    walk.tail_done();
    gs.records = walk.nrecords(), gs.selected = walk.sel, gs.out_bytes = walk.out_bytes;
    ctx->gcstats = bzh_grep_context_stats{walk.sel, 0, 0, 0};
    return BZH_OK;
}

// Bytes and entries have followed the stream to the caller's arrays; the tail's entry, the counts, and whether the rooms sufficed.
int GrepSink::report(bzh_ctx *ctx, size_t *nrecs, uint64_t *out_total)
{
    if (tail_ent_due) memcpy(&ent[sel() - 1], &tail_ent, sizeof tail_ent);
    *nrecs = (size_t)sel();
    *out_total = out_bytes();
    if (overflow()) {
        bzh_set_error(ctx, "grep: %llu records of %llu bytes, room for %llu and %llu", (unsigned long long)sel(),
                      (unsigned long long)out_bytes(), (unsigned long long)walk.max, (unsigned long long)walk.cap);
        return BZH_E_CAP;
    }
    return BZH_OK;
}
