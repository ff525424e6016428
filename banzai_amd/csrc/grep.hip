// grep.hip -- the records of decoded bytes in HBM that hold a byte string, compacted into the caller's buffer (bzh_grep*): the two
// passes over the tiles of a window, the scan between them, the staging buffer the decoders expand into and the carry between two
// windows (the windows: grep_plan.h; what one thread, one tile and the scan do: grep_core.h).  The text never leaves the device:
// what comes back is five words a window, and the selected records.
#include "common.h"
#include "grep_core.h"

static_assert(sizeof(bzh_grep_entry) == 32 && sizeof(BzgEntry) == sizeof(bzh_grep_entry), "an entry is four words");
static_assert(sizeof(BzgTile) == 32 && sizeof(BzgBase) == 24, "the tile tables");

struct GfPat { // the pattern, by value in the kernel's arguments
    uint32_t w[BZF_MAX_PATTERN / 4];
};

struct GfArgs {
    const uint8_t *d; // 16-byte aligned
    BzgWindow win;
    uint32_t plen, delim;
    uint32_t head, hmask; // the filter's word and mask (search_core.h)
    BzgTile *tile;        // [tiles] pass one writes, the scan completes, pass two reads
    const BzgBase *base;  // [tiles] the scan: what lies in front of every tile
    uint8_t *out;         // the caller's bytes (null: only entries are asked for); 4-byte aligned
    BzgEntry *ent;        // the window's entries [0, selected) (null: only bytes are asked for)
};

// A thread's 16 bytes at position p0 of d[0, n).  Inside the text: one aligned 16-byte load.  At its end: the aligned 4-byte words
// that begin in front of n, zeros behind them -- no read goes past the word that holds byte n - 1.
__device__ __forceinline__ uint4 gf_load16(const uint8_t *d, uint64_t n, uint64_t p0)
{
    if (p0 + 16 <= n) return *reinterpret_cast<const uint4 *>(d + p0);
    uint4 v;
    v.x = p0 < n ? *reinterpret_cast<const uint32_t *>(d + p0) : 0u;
    v.y = p0 + 4 < n ? *reinterpret_cast<const uint32_t *>(d + p0 + 4) : 0u;
    v.z = p0 + 8 < n ? *reinterpret_cast<const uint32_t *>(d + p0 + 8) : 0u;
    v.w = p0 + 12 < n ? *reinterpret_cast<const uint32_t *>(d + p0 + 12) : 0u;
    return v;
}

// One workgroup a tile of 4,096 positions, 16 a thread; the tile, the halo behind it and the pattern are staged in LDS as in
// search_tiles.  GATHER false: the tile's record (BzgTile), one plain store -- no atomics; grep_scan joins the tiles.  GATHER true,
// in tiles that hold selected bytes: the same masks again, the selection of every byte, the selected ones compacted in LDS and
// written to out[out_base + base.out ..) -- bytes of this tile only, to addresses no other workgroup writes: words inside the run,
// single bytes at its two ends -- and an entry from every thread that holds a selected record's delimiter.
template <bool GATHER>
__global__ void __launch_bounds__(BZF_THREADS) grep_tiles(GfArgs a, GfPat p)
{
    __shared__ __attribute__((aligned(16))) uint8_t tile[BZF_TILE + BZF_MAX_PATTERN];
    __shared__ __attribute__((aligned(4))) uint8_t pat[BZF_MAX_PATTERN];
    __shared__ BzgShared sh;
    const uint32_t tid = threadIdx.x;
    BzgTile x{};
    BzgBase base{};
    if (GATHER) {
        x = a.tile[blockIdx.x];
        if (x.bytes == 0) return; // (the same for every thread; a selected record's delimiter is one of its bytes)
        base = a.base[blockIdx.x];
    }
    const uint64_t n = a.win.n, t0 = (uint64_t)blockIdx.x * BZF_TILE, p0 = t0 + tid * BZF_ITEMS;
    if (tid < BZF_MAX_PATTERN / 4) reinterpret_cast<uint32_t *>(pat)[tid] = p.w[tid];
    const uint4 own = gf_load16(a.d, n, p0);
    *reinterpret_cast<uint4 *>(tile + tid * BZF_ITEMS) = own;
    if (tid * BZF_ITEMS < a.plen - 1) // the halo: the head of the next tile, as far as a match that starts in this one can reach
        *reinterpret_cast<uint4 *>(tile + BZF_TILE + tid * BZF_ITEMS) = gf_load16(a.d, n, t0 + BZF_TILE + tid * BZF_ITEMS);
    __syncthreads();
    const uint32_t next = *reinterpret_cast<const uint32_t *>(tile + tid * BZF_ITEMS + BZF_ITEMS); // (thread 255: the halo's first word, or what lies there)
    BzgThread t;
    bzg_masks(t, a.win, p0, own.x, own.y, own.z, own.w, next, a.delim, a.head, a.hmask);
    if (a.plen > 4) {
        uint32_t cand = t.hm;
        t.hm = 0;
        while (cand) {
            const uint32_t k = (uint32_t)__ffs((int)cand) - 1u;
            cand &= cand - 1u;
            if (bzf_verify(tile + tid * BZF_ITEMS + k, pat, a.plen)) t.hm |= 1u << k;
        }
    }
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

// ---- host side ---------------------------------------------------------------------------------------------------
// The passes over the window w of d (16-byte aligned; w.n bytes lie there, and the aligned word that holds the last of them).  One
// wait, for the window's totals; bytes and entries follow the stream and are there after the call's last wait.
static int grep_window_run(bzh_ctx *ctx, GrepSink &g, const uint8_t *d, const BzgWindow &w, uint64_t bytes)
{
    hipStream_t st = ctx->stream;
    bzh_grep_stats &gs = ctx->gstats;
    const uint64_t tiles64 = (w.n + BZF_TILE - 1) / BZF_TILE;
    if (tiles64 > 0x7FFFFFFFull) {
        bzh_set_error(ctx, "grep: a window of %llu bytes is beyond one launch", (unsigned long long)w.n);
        return BZH_E_ARG;
    }
    const uint32_t tiles = (uint32_t)tiles64;
    gs.windows++;
    gs.tiles += tiles;
    uint64_t totals[BZG_TOTALS] = {0, 0, 0, w.t_lo, w.open_hit};
    if (tiles && w.p_hi > w.p_lo) {
        BzgTile *tile = nullptr;
        BzgBase *base = nullptr;
        uint64_t *d_tot = nullptr;
        BZH_TRY(reserve_cut(ctx, ctx->grep_tab, "the grep's tile tables", grow_mib,
                            [&](Carver &c) { c.put(tile, tiles), c.put(base, tiles), c.put(d_tot, BZG_TOTALS); }));
        GfPat p;
        memcpy(p.w, g.pat, sizeof p.w);
        GfArgs a{d, w, g.plen, g.delim, bzf_head_word(g.pat, g.plen), bzf_head_mask(g.plen), tile, base, nullptr, nullptr};
        grep_tiles<false><<<dim3(tiles), BZF_THREADS, 0, st>>>(a, p);
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
            grep_tiles<true><<<dim3(tiles), BZF_THREADS, 0, st>>>(a, p);
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

// The staging buffer for a window of `bytes` decoded bytes: grown to the carry and to them (whole blocks, at least one), the carry
// put in front of the new bytes.  *d_stage lies as far inside the buffer as the carry exceeds BZF_FRONT: the decoders expand at
// *d_stage + BZF_FRONT, as for a search.
int grep_sink_room(bzh_ctx *ctx, GrepSink &g, uint64_t bytes, uint8_t **d_stage)
{
    const uint64_t carry = g.walk.carry, extra = bzg_front_extra(carry, BZF_FRONT);
    uint8_t *base = nullptr;
    BZH_TRY(reserve_cut(ctx, ctx->search_ws, "the grep's staging", grow_mib, [&](Carver &c) { c.put(base, (size_t)(extra + BZF_FRONT + bytes + 16)); }));
    ctx->gstats.staging_peak = std::max<uint64_t>(ctx->gstats.staging_peak, ctx->search_ws.cap);
    g.front = extra + BZF_FRONT;
    if (carry) // (kept apart between two windows: the staging buffer may have moved)
        HIP_TRY(ctx, hipMemcpyAsync(base + g.front - carry, ctx->grep_carry, (size_t)carry, hipMemcpyDeviceToDevice, ctx->stream));
    *d_stage = base + extra;
    return BZH_OK;
}

// The window grep_sink_room made room for has been expanded and verified: the passes, then everything behind the last delimiter
// they processed is kept as the carry.  (The copy is queued behind the window's wait -- where the tail starts is one of its totals
// -- and reserve() waits for the stream before it frees, so the staging buffer outlives it.)
int grep_sink_window(bzh_ctx *ctx, GrepSink &g, uint64_t bytes)
{
    const uint8_t *base = ctx->search_ws.p;
    BZH_TRY(grep_window_run(ctx, g, base, g.walk.window(g.front, bytes, false), bytes));
    const uint64_t keep = g.walk.carry;
    BZH_TRY(ctx->grep_carry.reserve(ctx, (size_t)keep + 16, "the grep's carry", grow_mib));
    if (keep) HIP_TRY(ctx, hipMemcpyAsync(ctx->grep_carry, g.tail, (size_t)keep, hipMemcpyDeviceToDevice, ctx->stream));
    g.tail = ctx->grep_carry;
    return BZH_OK;
}

// Decoded bytes that already lie in HBM: one window, no staging, no carry.
int grep_raw_run(bzh_ctx *ctx, GrepSink &g, const uint8_t *d_raw, size_t n)
{
    g.front = 0;
    return grep_window_run(ctx, g, d_raw, g.walk.window(0, n, true), n);
}

// Behind the last window: the bytes held back are processed where they lie, in the carry; then the open tail, if it is a selected
// record, goes out in one copy.  *tail_entry: the caller stores the tail's entry at ent[walk.sel - 1] behind its last wait.
int grep_finish(bzh_ctx *ctx, GrepSink &g, bool *tail_entry)
{
    *tail_entry = false;
    if (g.walk.held) BZH_TRY(grep_window_run(ctx, g, ctx->grep_carry, g.walk.window(g.walk.carry, 0, true), 0));
    bool copy = false;
    g.walk.tail_rooms(&copy, tail_entry);
    g.tail_ent = g.walk.tail_entry();
    if (copy)
        HIP_TRY(ctx, hipMemcpyAsync(g.d_out + g.walk.out_bytes, g.tail, (size_t)g.walk.carry, hipMemcpyDeviceToDevice, ctx->stream));
    g.walk.tail_done();
    bzh_grep_stats &gs = ctx->gstats;
    gs.records = g.walk.nrecords(), gs.selected = g.walk.sel, gs.out_bytes = g.walk.out_bytes;
    return BZH_OK;
}
