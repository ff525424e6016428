// search.hip -- every occurrence of a byte string in decoded bytes that lie in HBM (bzh_search*): the kernel, the two passes over
// one window, and the search as a ScanSink (common.h: the decoders' WindowSink, and what the routes of api.hip call once a call),
// with the two host helpers it shares with the grep's sink: the staging room and the tile count.  The windows and the carry: search_plan.h; the tile front -- load, staging, filter, verify,
// shared with grep_tiles -- and what one thread does behind it: search_core.h.  The bytes never leave the device: what comes back
// is a word a window, and the hits.
#include "common.h"
#include "search_core.h"
#include "matcher_pick.h"

static_assert(BZF_MAX_PATTERN == BZH_SEARCH_MAX_PATTERN, "search_core.h and bzhip.h name the same bound");
static_assert(BZF_FRONT % 16 == 0 && BZF_FRONT >= BZF_MAX_PATTERN, "a window begins aligned, its carry in front of it");
static_assert(sizeof(bzh_hit) == 16 && sizeof(BzfHit) == sizeof(bzh_hit), "a hit is two words");
static_assert(sizeof(bzh_set_hit) == 24 && sizeof(BzmHit) == sizeof(bzh_set_hit), "a set's hit is three");

struct SfArgs {
    const uint8_t *d; // 16-byte aligned
    BzfWindow win;
    uint32_t records;
    uint32_t *thits, *tdel;        // [tiles] pass one: hits and delimiters of every tile
    const uint64_t *hbase, *dbase; // [tiles] search_scan: those in front of every tile
    void *out;                     // the window's hit slots [0, win.emit): the matcher's Hit
};

// One workgroup a tile of 4,096 positions, 16 a thread.  The tile and the halo behind it are staged in LDS, and what the matcher M
// keeps beside them (patset_core.h: BzfOne, the single pattern -- every lane reads the same byte of it; BzmMatcher, a set).  EMIT false: the tile's hits and delimiters, reduced over the workgroup, a plain store each -- no
// atomics; search_scan sums the tiles.  EMIT true: the same tests again, in tiles that hold a hit in front of the caller's bound,
// and every hit whose rank in the window is below win.emit stores itself at its rank: the output ascends, and "the first max" costs
// nothing.  Stores: the tile's two words, or hit slots below win.emit.
template <bool EMIT, class M>
__global__ void __launch_bounds__(BZF_THREADS) search_tiles(SfArgs a, M m)
{
    __shared__ __attribute__((aligned(16))) uint8_t tile[BZF_TILE + BZF_MAX_PATTERN];
    __shared__ typename M::Shared msh;
    __shared__ uint32_t lds[8];
    const uint32_t tid = threadIdx.x;
    if (EMIT && (a.thits[blockIdx.x] == 0 || a.hbase[blockIdx.x] >= a.win.emit)) return; // (the same for every thread)
    const uint64_t n = a.win.n, t0 = (uint64_t)blockIdx.x * BZF_TILE, p0 = t0 + tid * BZF_ITEMS;
    const BzfVec own = m.stage(a.d, n, t0, tid, tile, msh);
    __syncthreads();
    uint32_t hm;
    const uint32_t nh = m.count16(own, tid, p0, tile, msh, bzf_range_mask16(p0, a.win.s_lo, a.win.s_hi), &hm);
    const uint32_t dm = a.records ? bzf_eq_mask16(own.x, own.y, own.z, own.w, m.delim()) & bzf_range_mask16(p0, a.win.d_lo, n) : 0u;
    const uint32_t nd = (uint32_t)__popc(dm);
    if (!EMIT) {
        const uint32_t sh = wave_reduce_add(nh), sd = wave_reduce_add(nd);
        if ((tid & 63u) == 0) lds[tid >> 6] = sh, lds[4 + (tid >> 6)] = sd;
        __syncthreads();
        if (tid == 0) {
            a.thits[blockIdx.x] = lds[0] + lds[1] + lds[2] + lds[3];
            a.tdel[blockIdx.x] = lds[4] + lds[5] + lds[6] + lds[7];
        }
        return;
    }
    uint32_t th, td;
    const uint32_t h0 = block_excl_add(nh, lds, &th);
    const uint32_t d0 = a.records ? block_excl_add(nd, lds, &td) : 0u;
    uint64_t rank = a.hbase[blockIdx.x] + h0;
    while (hm) {
        const uint32_t k = (uint32_t)__ffs((int)hm) - 1u;
        hm &= hm - 1u;
        if (rank < a.win.emit) { // (a start's hits ascend: none of a start whose first is not stored is)
            const uint64_t pos = p0 + k;
            uint64_t rec = 0;
            if (a.records) {
                if (pos >= a.win.d_lo) {
                    rec = a.win.rec_base + a.dbase[blockIdx.x] + d0 + bzf_delims_before(dm, k);
                } else { // a start in the carry: the delimiters between it and d_lo were counted by the window before
                    const uint32_t gap = (uint32_t)min(a.win.d_lo - pos, (uint64_t)BZF_MAX_PATTERN); // (the halo holds them: max_len - 1 bytes, one more with a look-ahead)
                    uint32_t c = 0;
                    for (uint32_t j = 0; j < gap; j++) c += tile[tid * BZF_ITEMS + k + j] == m.delim();
                    rec = a.win.rec_base - c;
                }
            }
            rank = m.emit1(msh, tile + tid * BZF_ITEMS + k, pos, a.win.off_base + pos, rec, static_cast<typename M::Hit *>(a.out), rank, a.win.emit);
        } else {
            break; // (the ranks ascend)
        }
    }
}

// The tiles of a window summed in one workgroup: thread t takes the tiles [t c, t c + c), c = ceil(tiles / threads); hbase / dbase =
// the hits and delimiters in front of every tile, totals[0 .. 1] those of the window.
__global__ void __launch_bounds__(BZF_THREADS) search_scan(const uint32_t *thits, const uint32_t *tdel, uint32_t tiles, uint64_t *hbase,
                                                            uint64_t *dbase, uint64_t *totals)
{
    __shared__ uint64_t sh[BZF_THREADS], sd[BZF_THREADS];
    const uint32_t c = (tiles + BZF_THREADS - 1) / BZF_THREADS, lo = min(tiles, threadIdx.x * c), hi = min(tiles, lo + c);
    uint64_t h = 0, d = 0;
    for (uint32_t t = lo; t < hi; t++) h += thits[t], d += tdel[t];
    sh[threadIdx.x] = h, sd[threadIdx.x] = d;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t rh = 0, rd = 0;
        for (uint32_t k = 0; k < BZF_THREADS; k++) {
            const uint64_t vh = sh[k], vd = sd[k];
            sh[k] = rh, sd[k] = rd;
            rh += vh, rd += vd;
        }
        totals[0] = rh, totals[1] = rd;
    }
    __syncthreads();
    h = sh[threadIdx.x], d = sd[threadIdx.x];
    for (uint32_t t = lo; t < hi; t++) {
        hbase[t] = h, dbase[t] = d;
        h += thits[t], d += tdel[t];
    }
}

// ---- host side: what the search's and the grep's sinks share --------------------------------------------------------------
// The staging buffer for a window of `bytes` decoded bytes behind a carry of `carry` bytes: grown to them (whole blocks, at least
// one, so a block above the target grows it), the carry copied in front of the new bytes.  The decoders expand at
// *d_stage + BZF_FRONT = staging position *front; *d_stage lies as far inside the buffer as the carry exceeds BZF_FRONT (a search's
// never does).
int scan_room(bzh_ctx *ctx, const char *what, uint64_t carry, uint64_t bytes, uint64_t *staging_peak, uint8_t **d_stage, uint64_t *front)
{
    const uint64_t extra = bzg_front_extra(carry, BZF_FRONT);
    uint8_t *base = nullptr;
    BZH_TRY(reserve_cut(ctx, ctx->search_ws, what, grow_mib, [&](Carver &c) { c.put(base, (size_t)(extra + BZF_FRONT + bytes + 16)); }));
    *staging_peak = std::max<uint64_t>(*staging_peak, ctx->search_ws.cap);
    *front = extra + BZF_FRONT;
    if (carry) // (kept apart between two windows: the staging buffer may have moved)
        HIP_TRY(ctx, hipMemcpyAsync(base + *front - carry, ctx->scan_carry, (size_t)carry, hipMemcpyDeviceToDevice, ctx->stream));
    *d_stage = base + extra;
    return BZH_OK;
}

// The tiles of a window of n bytes, one launch's worth at most; the window and they are counted.  who: "search" or "grep".
int scan_tiles(bzh_ctx *ctx, const char *who, uint64_t n, uint64_t *windows, uint64_t *tiles_sum, uint32_t *tiles)
{
    const uint64_t tiles64 = (n + BZF_TILE - 1) / BZF_TILE;
    if (tiles64 > 0x7FFFFFFFull) {
        bzh_set_error(ctx, "%s: a window of %llu bytes is beyond one launch", who, (unsigned long long)n);
        return BZH_E_ARG;
    }
    *tiles = (uint32_t)tiles64;
    (*windows)++;
    *tiles_sum += tiles64;
    return BZH_OK;
}

// ---- host side: the search ---------------------------------------------------------------------------------------------------------
// The two passes over the window w of d (16-byte aligned; w.n bytes lie there, and the aligned word that holds the last of them).
// One wait, for the window's two totals; the hits follow the stream to the caller's array and are there after the call's last wait.
// lim: where a set's matches end (search_plan.h: BzmSetWalk).
static int search_window_run(bzh_ctx *ctx, SearchSink &s, const uint8_t *d, BzfWindow w, uint64_t lim, uint64_t bytes, bool last)
{
    hipStream_t st = ctx->stream;
    bzh_search_stats &ss = ctx->sstats;
    const BzfPick pick{lim, w.n, 0 - w.off_base, BZR_LOOK_EDGE}; // (output offset 0 lies at position 0 - off_base: the text's edge stands in front of it)
    uint32_t tiles;
    BZH_TRY(scan_tiles(ctx, "search", w.n, &ss.windows, &ss.tiles, &tiles));
    uint64_t totals[2] = {0, 0};
    if (tiles && (w.s_hi > w.s_lo || s.records)) {
        uint32_t *thits = nullptr, *tdel = nullptr;
        uint64_t *hbase = nullptr, *dbase = nullptr, *d_tot = nullptr;
        BZH_TRY(reserve_cut(ctx, ctx->search_tab, "the search's tile tables", grow_mib, [&](Carver &c) {
            c.put(hbase, tiles), c.put(dbase, tiles), c.put(d_tot, 2), c.put(thits, tiles), c.put(tdel, tiles);
        }));
        SfArgs a{d, w, s.records ? 1u : 0u, thits, tdel, hbase, dbase, nullptr};
        pick_matcher(s.pat, s.set, s.delim, pick, [&](const auto &m) { search_tiles<false><<<dim3(tiles), BZF_THREADS, 0, st>>>(a, m); });
        search_scan<<<dim3(1), BZF_THREADS, 0, st>>>(thits, tdel, tiles, hbase, dbase, d_tot);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(totals, d_tot, sizeof totals, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, bzh_stream_wait(st));
        const uint64_t emit = s.walk.emit(totals[0]);
        if (emit) {
            const size_t hs = s.hit_size();
            BZH_TRY(ctx->search_out.reserve(ctx, (size_t)emit * hs, "the search's hits", grow_mib));
            a.win.emit = emit;
            a.out = ctx->search_out.p;
            pick_matcher(s.pat, s.set, s.delim, pick, [&](const auto &m) { search_tiles<true><<<dim3(tiles), BZF_THREADS, 0, st>>>(a, m); });
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipMemcpyAsync((uint8_t *)s.hits + (size_t)s.walk.rank * hs, a.out, (size_t)emit * hs, hipMemcpyDeviceToHost, st));
        }
    }
    if (s.set) s.walk.advance_set(bytes, totals[0], totals[1], last);
    else s.walk.advance(bytes, totals[0], totals[1]);
    ss.hits = s.walk.rank;
    return BZH_OK;
}

int SearchSink::room(bzh_ctx *ctx, uint64_t bytes, uint8_t **d_stage)
{
    uint64_t at; // (front: a search's carry is shorter)
    return scan_room(ctx, "the search's staging", walk.carry, bytes, &ctx->sstats.staging_peak, d_stage, &at);
}

// The two passes, and the window's tail is kept as the carry.
int SearchSink::window(bzh_ctx *ctx, uint64_t bytes)
{
    const uint8_t *base = ctx->search_ws.p;
    uint64_t lim = 0; // (of a set's window)
    const BzfWindow w = set ? walk.window_set(bytes, false, &lim) : walk.window(bytes);
    const uint64_t keep = set ? walk.carry_after_set(bytes) : walk.carry_after(bytes);
    if (keep) { // [n - keep, n): read before the passes' wait, written where no pass looks
        BZH_TRY(ctx->scan_carry.reserve(ctx, BZF_MAX_PATTERN + 16, "the search's carry")); // (with assertions up to 257 bytes)
        HIP_TRY(ctx, hipMemcpyAsync(ctx->scan_carry, base + w.n - keep, (size_t)keep, hipMemcpyDeviceToDevice, ctx->stream));
    }
    return search_window_run(ctx, *this, base, w, lim, bytes, false);
}

// Decoded bytes that already lie in HBM: one window, no staging, no carry.
int SearchSink::raw(bzh_ctx *ctx, const uint8_t *d_raw, size_t n)
{
    walk.begin(plen(), 0, max, 0, n, 0, 0);
    walk.begin_look(look_behind, look_ahead);
    uint64_t lim = 0;
    const BzfWindow w = set ? walk.window_set(n, true, &lim) : walk.window(n);
    return search_window_run(ctx, *this, d_raw, w, lim, n, true);
}

// Behind the last window of a set search: the starts held back are processed where they lie, in the carry -- a window without new
// bytes, its text the carry, every delimiter of which has been counted.  (Behind raw() nothing is carried.)
int SearchSink::finish(bzh_ctx *ctx)
{
    if (!set || !walk.carry) return BZH_OK;
    walk.front = walk.carry;
    uint64_t lim = 0;
    const BzfWindow w = walk.window_set(0, true, &lim);
    return search_window_run(ctx, *this, ctx->scan_carry, w, lim, 0, true);
}

// The hits have followed the stream to the caller's array; the count, and whether the array had room for them.
int SearchSink::report(bzh_ctx *ctx, size_t *nhits, uint64_t *)
{
    *nhits = (size_t)walk.rank;
    if (walk.rank > max && max) {
        bzh_set_error(ctx, "search: %llu hits, room for %llu", (unsigned long long)walk.rank, (unsigned long long)max);
        return BZH_E_CAP;
    }
    return BZH_OK;
}
