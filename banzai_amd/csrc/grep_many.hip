// grep_many.hip -- the grep over many texts that lie in one buffer in HBM with walls between them (bzh_grep_many*): for every text
// what bzh_grep returns for it alone.  One workgroup per VIRTUAL TILE -- a (segment, tile of the buffer) pair of the table
// grep_many_plan.h builds -- runs grep_tiles' phases (grep_core.h) behind the tile front (search_core.h, patset_core.h,
// regex_core.h) with the segment's window and the matcher rebound to the segment (grep_many_core.h); the scan between the two
// passes is grep_scan's phases with the segments' walls in it.  No atomics; every workgroup writes only bytes of its own tile; one
// host wait before the gather.  The route as a GrepSink method (common.h): GrepSink::raw_many.
#include "common.h"
#include "grep_many_plan.h"
#include "matcher_pick.h"

static_assert(sizeof(BzgmSeg) == 24 && sizeof(BzgmRow) == 8, "the segment table, the virtual tile table");

struct GmArgs {
    const uint8_t *d; // 16-byte aligned
    const BzgmRow *row;
    const BzgmSeg *seg;
    BzgTile *tile;       // [rows] pass one writes, the scan completes, pass two reads
    const BzgBase *base; // [rows] the scan: what lies in front of every virtual tile, in the call
    uint8_t *out;        // the caller's bytes (null: only entries are asked for); 4-byte aligned
    BzgEntry *ent;       // the call's entries [0, selected) (null: only bytes are asked for)
    uint32_t plen;       // of a single pattern (its starts end plen - 1 in front of the segment's end); else 1
    uint32_t invert;
};

// grep_tiles for virtual tile blockIdx.x: its row names the segment and the tile; the window is the segment's, the copy of the
// matcher in this kernel's arguments is rebound to it, and the segment's last byte closes a record.  Reads: the tile and its halo
// to the aligned word that holds byte hi - 1 of the segment (bytes of a neighbour in front of lo are loaded and masked out of
// every mask); with assertions the one byte in front of the tile, which lies inside the buffer.  Writes: as grep_tiles.
template <bool GATHER, class M>
__global__ void __launch_bounds__(BZF_THREADS) grep_many_tiles(GmArgs a, M m)
{
    __shared__ __attribute__((aligned(16))) uint8_t tile[BZF_TILE + BZF_MAX_PATTERN];
    __shared__ typename M::Shared msh;
    __shared__ BzgShared sh;
    const uint32_t tid = threadIdx.x, v = blockIdx.x;
    const BzgmRow r = a.row[v];
    const BzgmSeg s = a.seg[r.seg];
    BzgTile x{};
    BzgBase base{};
    if (GATHER) {
        x = a.tile[v];
        if (x.bytes == 0) return; // (the same for every thread)
        base = bzgm_base(a.base, v, s);
    }
    const BzgWindow w = bzgm_window(s, a.plen, a.invert);
    bzgm_rebind(m, s.lo, s.hi);
    const uint64_t t0 = (uint64_t)r.tile * BZF_TILE, p0 = t0 + tid * BZF_ITEMS;
    const BzfVec own = m.stage(a.d, w.n, t0, tid, tile, msh);
    __syncthreads();
    BzgThread t;
    const uint32_t starts = M::BY_LIM ? bzf_range_mask16(p0, w.p_lo, w.p_hi) : bzg_starts(w, p0);
    bzg_masks(t, w, p0, own, m.delim(), m.match16(own, tid, p0, tile, msh, starts));
    bzgm_close(t, w, p0);
    bzg_local(t, w.invert);
    bzg_count_p0(sh, tid, t);
    __syncthreads();
    for (uint32_t k = 0; k < 8; k++) {
        bzg_step_f(sh, tid, k);
        __syncthreads();
    }
    if (!GATHER) {
        bzg_count_p1(sh, tid, t, w.invert);
        __syncthreads();
        for (uint32_t k = 0; k < 8; k++) {
            bzg_step_s(sh, tid, k);
            __syncthreads();
        }
        if (tid == 0) {
            BzgTile o;
            bzg_count_p2(sh, o);
            a.tile[v] = o;
        }
        return;
    }
    bool sel_first;
    bzg_gather_p1(sh, tid, t, x, w.invert, &sel_first);
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
    uint8_t *dst = a.out ? a.out + base.out : nullptr;
    const uint32_t shift = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3u);
    bzg_gather_p3(sh, tid, r.tile, t, x, base, w, tile + tid * BZF_ITEMS, sm, sdm, shift, dst != nullptr, a.ent);
    if (!dst) return;
    __syncthreads();
    bzg_gather_p4(sh, tid, dst, shift, x.bytes);
}

// grep_scan over the virtual tiles, as a segmented scan: one workgroup, every thread a run of consecutive rows.  totals: the
// call's BZG_TOTALS words, and behind them one row of BZGM_TOTALS words per segment.
__global__ void __launch_bounds__(BZF_THREADS) grep_many_scan(BzgTile *tile, uint32_t rows, BzgBase *base, const BzgmRow *row, const BzgmSeg *seg,
                                                              uint32_t segs, uint32_t invert, uint64_t *totals)
{
    __shared__ BzgScanShared sh;
    const uint32_t tid = threadIdx.x;
    const BzgManyTexts texts{row, seg};
    BzgWindow w{};
    w.invert = invert;
    bzg_scan_a(sh, tid, tile, rows, texts);
    __syncthreads();
    if (tid == 0) bzg_scan_b(sh, w, totals); // (the first row is a segment's first: what the window carries in is never used)
    __syncthreads();
    bzg_scan_c(sh, tid, tile, rows, w, texts);
    __syncthreads();
    if (tid == 0) bzg_scan_d(sh);
    __syncthreads();
    bzg_scan_e(sh, tid, tile, rows, w, texts);
    __syncthreads();
    if (tid == 0) bzg_scan_f(sh, totals);
    __syncthreads();
    bzg_scan_g(sh, tid, tile, rows, base);
    __syncthreads(); // (base and totals are this workgroup's own stores)
    for (uint32_t k = tid; k < segs; k += BZF_THREADS) bzgm_totals(seg, k, base, rows, totals, totals + BZG_TOTALS);
}

// ---- host side ---------------------------------------------------------------------------------------------------
// The one segmented pass over d_raw (16-byte aligned; every segment's bytes lie there, and the aligned word that holds the last of
// them).  One wait, for the call's and the segments' totals; bytes and entries follow the stream.
int GrepSink::raw_many(bzh_ctx *ctx, const uint8_t *d_raw, const BzgmPlan &plan, uint64_t *seg_totals)
{
    hipStream_t st = ctx->stream;
    bzh_grep_stats &gs = ctx->gstats;
    const size_t segs = plan.seg.size();
    const uint32_t rows = (uint32_t)plan.rows;
    memset(seg_totals, 0, segs * BZGM_TOTALS * sizeof(uint64_t));
    gs.windows = 1, gs.tiles = rows;
    if (!rows) return BZH_OK;
    BzgmSeg *d_seg = nullptr;
    BzgmRow *d_row = nullptr;
    uint64_t *d_tot = nullptr;
    BzgTile *tile = nullptr;
    BzgBase *base = nullptr;
    const size_t words = BZG_TOTALS + segs * BZGM_TOTALS;
    BZH_TRY(reserve_cut(ctx, ctx->grep_many_tab, "the segment tables of a grep over many inputs", grow_mib,
                        [&](Carver &c) { c.put(d_seg, segs), c.put(d_tot, words), c.put(d_row, rows); }));
    BZH_TRY(reserve_cut(ctx, ctx->grep_tab, "the grep's tile tables", grow_mib, [&](Carver &c) { c.put(tile, rows), c.put(base, rows); }));
    HIP_TRY(ctx, hipMemcpyAsync(d_seg, plan.seg.data(), segs * sizeof(BzgmSeg), hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_row, plan.row.data(), (size_t)rows * sizeof(BzgmRow), hipMemcpyHostToDevice, st));
    // (the matcher's own bounds are rebound per segment in the kernel; what is given here is never used)
    const BzfPick pick{0, 0, 0, (uint32_t)BZR_LOOK_EDGE};
    GmArgs a{d_raw, d_row, d_seg, tile, base, nullptr, nullptr, set ? 1u : pat.plen, walk.invert};
    pick_matcher(pat, set, delim, pick, [&](const auto &m) { grep_many_tiles<false><<<dim3(rows), BZF_THREADS, 0, st>>>(a, m); });
    grep_many_scan<<<dim3(1), BZF_THREADS, 0, st>>>(tile, rows, base, d_row, d_seg, (uint32_t)segs, walk.invert, d_tot);
    HIP_TRY(ctx, hipGetLastError());
    std::vector<uint64_t> tot(words);
    HIP_TRY(ctx, hipMemcpyAsync(tot.data(), d_tot, words * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, bzh_stream_wait(st));
    memcpy(seg_totals, tot.data() + BZG_TOTALS, segs * BZGM_TOTALS * sizeof(uint64_t));
    // the walk's totals, as finish() and report() read them: nothing is carried, nothing is held back
    walk.recs = tot[BZG_T_DEL], walk.sel = tot[BZG_T_SEL], walk.out_bytes = tot[BZG_T_BYTES];
    const BzgmRooms rooms{walk.want_out, walk.want_ent, walk.cap, walk.max};
    walk.fits = rooms.fits(walk.out_bytes, walk.sel);
    if (rooms.gather(walk.out_bytes, walk.sel)) {
        a.out = walk.want_out ? d_out : nullptr;
        if (walk.want_ent) {
            BZH_TRY(ctx->grep_ent.reserve(ctx, (size_t)walk.sel * sizeof(BzgEntry), "the grep's entries", grow_mib));
            a.ent = ctx->grep_ent.as<BzgEntry>();
        }
        pick_matcher(pat, set, delim, pick, [&](const auto &m) { grep_many_tiles<true><<<dim3(rows), BZF_THREADS, 0, st>>>(a, m); });
        HIP_TRY(ctx, hipGetLastError());
        if (a.ent) HIP_TRY(ctx, hipMemcpyAsync(ent, a.ent, (size_t)walk.sel * sizeof(BzgEntry), hipMemcpyDeviceToHost, st));
    }
    return BZH_OK;
}
