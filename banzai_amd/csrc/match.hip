// match.hip -- the matched parts alone (grep -o): the non-overlapping, leftmost-longest matches of decoded bytes in HBM, their bytes
// compacted back to back into the caller's buffer (bzh_match*).  Five launches a window, as the context grep's: match_tiles runs
// the matcher and writes every tile's map, match_scan gives every tile its entry, match_select<false> counts what every tile
// selects, match_sum puts the sums in front of every tile, match_select<true> writes entries and bytes.  The phases: match_core.h;
// the windows and the cursor between them: match_plan.h; the tile front and the matchers: search_core.h, matcher_pick.h.  One wait
// a window, for its totals.  No atomics; every workgroup stores only what belongs to its own tile.
#include "common.h"
#include "match_core.h"
#include "matcher_pick.h"

static_assert(sizeof(bzh_match_entry) == 32 && sizeof(MtEntry) == sizeof(bzh_match_entry), "an entry is four words");
static_assert(sizeof(MtTile) == 16 && sizeof(MtCount) == 16 && sizeof(MtBase) == 24, "the tile tables");

struct MfArgs {
    const uint8_t *d; // 16-byte aligned
    MtWindow win;
    uint32_t records;
    MtTile *tile;     // [tiles] pass one writes, the scan adds the entry
    uint8_t *map;     // [tiles * 256] pass one: the map of every open tile
    uint16_t *hits;   // [tiles * 256] pass one: every thread's match starts
    uint8_t *lens;    // [tiles * 4096] pass one: L - 1 at every match start
    MtCount *cnt;     // [tiles] pass two
    MtBase *base;     // [tiles] del: the scan; cnt, bytes: the sum
    uint8_t *out;     // the caller's bytes (null: not asked for)
    MtEntry *ent;     // the window's entries [0, selected) (null: not asked for)
};

// the levels of a tile up to y (match_core.h); a barrier behind every round
__device__ __forceinline__ void match_levels(MtShared &sh, uint32_t tid, uint32_t hm, const BzfVec &len)
{
    mt_local(sh, tid, hm, len);
    __syncthreads();
    for (uint32_t r = 0; r < 4; r++) {
        mt_group_step(sh, tid, r);
        __syncthreads();
    }
}
__device__ __forceinline__ void match_sums(MtShared &sh, uint32_t tid)
{
    __syncthreads();
    for (uint32_t k = 0; k < 8; k++) {
        mt_sum_step(sh, tid, k);
        __syncthreads();
    }
}

// Pass one: one workgroup a tile of 4,096 positions, 16 a thread, behind the front it shares with search_tiles and grep_tiles.
// The matcher runs here and nowhere else but at the selected starts of the last pass: every thread's match starts and their
// lengths go into the tables, the tile's map is made in LDS.  A tile without a match is left at its first byte whatever the entry.
template <class M>
__global__ void __launch_bounds__(BZF_THREADS) match_tiles(MfArgs a, M m)
{
    __shared__ __attribute__((aligned(16))) uint8_t tile[BZF_TILE + BZF_MAX_PATTERN];
    __shared__ typename M::Shared msh;
    __shared__ MtShared sh;
    const uint32_t tid = threadIdx.x;
    const BzfWindow &w = a.win.w;
    const uint64_t t0 = (uint64_t)blockIdx.x * BZF_TILE, p0 = t0 + tid * BZF_ITEMS;
    const BzfVec own = m.stage(a.d, w.n, t0, tid, tile, msh);
    mt_init(sh, tid);
    __syncthreads();
    const uint32_t hm = m.match16(own, tid, p0, tile, msh, bzf_range_mask16(p0, w.s_lo, w.s_hi));
    BzfVec len{0, 0, 0, 0};
    for (uint32_t v = hm; v; v &= v - 1u) {
        const uint32_t k = (uint32_t)__ffs((int)v) - 1u;
        uint32_t pattern;
        const uint32_t l = m.longest1(msh, tile + tid * BZF_ITEMS + k, p0 + k, &pattern) - 1u;
        const uint32_t word = l << (8u * (k & 3u));
        if (k < 4) len.x |= word;
        else if (k < 8) len.y |= word;
        else if (k < 12) len.z |= word;
        else len.w |= word;
    }
    a.hits[(size_t)blockIdx.x * BZF_THREADS + tid] = (uint16_t)hm;
    if (hm) {
        *reinterpret_cast<BzfVec *>(a.lens + p0) = len;
        sh.any = 1; // (every writer stores the same word)
    }
    const uint32_t dm = a.records ? bzf_eq_mask16(own.x, own.y, own.z, own.w, m.delim()) & bzf_range_mask16(p0, w.d_lo, w.n) : 0u;
    mt_sum_put(sh, tid, (uint32_t)__popc(hm), 0, (uint32_t)__popc(dm));
    match_sums(sh, tid);
    MtTile o{mt_s_cnt(mt_sum_all(sh)), mt_s_del(mt_sum_all(sh)), MT_CONST, 0};
    if (sh.any) { // (the same for every thread)
        match_levels(sh, tid, hm, len);
        mt_map(sh, tid);
        __syncthreads();
        mt_map_open(sh, tid);
        __syncthreads();
        if (sh.open) a.map[(size_t)blockIdx.x * 256u + tid] = sh.map[tid], o.konst = 0;
        else o.konst = MT_CONST | sh.map[0];
    }
    if (tid == 0) a.tile[blockIdx.x] = o;
}

// The entry of every tile, one workgroup (match_core.h: the scan).  summ: [256 * 256] a row a thread.
__global__ void __launch_bounds__(BZF_THREADS) match_scan(MtTile *tile, const uint8_t *map, uint32_t tiles, MtBase *base, uint8_t *summ, uint64_t *totals)
{
    __shared__ MtScanShared sh;
    const uint32_t tid = threadIdx.x;
    mt_scan_a(sh, tid, tile, map, tiles, summ);
    __syncthreads();
    if (tid == 0) mt_scan_b(sh, summ, totals);
    __syncthreads();
    mt_scan_c(sh, tid, tile, map, tiles, base);
    __syncthreads();
    if (tid == 0) mt_scan_d(sh, totals);
}

struct MtNoMatcher { // the counting pass takes none
    using Shared = uint32_t;
};
// Passes two and three: the selection of the tile from the tables and its entry.  GATHER false: the tile's counts, no matcher and
// no text.  GATHER true, in tiles that select a match: the entries at their ranks and the bytes, compacted in LDS from the tile
// and its halo and written to out[out_base + base.bytes ..) -- bytes of matches that start in this tile only.
template <bool GATHER, class M>
__global__ void __launch_bounds__(BZF_THREADS) match_select(MfArgs a, M m)
{
    __shared__ __attribute__((aligned(16))) uint8_t tile[GATHER ? BZF_TILE + BZF_MAX_PATTERN : 16];
    __shared__ typename M::Shared msh;
    __shared__ MtShared sh;
    const uint32_t tid = threadIdx.x;
    const BzfWindow &w = a.win.w;
    const MtTile x = a.tile[blockIdx.x];
    if (!GATHER && x.cand == 0) { // (the same for every thread)
        if (tid == 0) a.cnt[blockIdx.x] = MtCount{0, 0, 0, 0};
        return;
    }
    uint32_t want = 0;
    if constexpr (GATHER) {
        want = a.cnt[blockIdx.x].bytes;
        if (want == 0) return; // (a selected match has a byte)
    }
    const uint64_t t0 = (uint64_t)blockIdx.x * BZF_TILE, p0 = t0 + tid * BZF_ITEMS;
    BzfVec own{0, 0, 0, 0};
    if constexpr (GATHER) own = m.stage(a.d, w.n, t0, tid, tile, msh);
    mt_init(sh, tid);
    const uint32_t hm = a.hits[(size_t)blockIdx.x * BZF_THREADS + tid];
    BzfVec len{0, 0, 0, 0};
    if (hm) len = *reinterpret_cast<const BzfVec *>(a.lens + p0);
    match_levels(sh, tid, hm, len);
    if (tid == 0) mt_group_entries(sh, x.entry);
    __syncthreads();
    if (tid < BZF_TILE / MT_GROUP) mt_seg_entries(sh, tid);
    __syncthreads();
    uint32_t bytes, last_end;
    const uint32_t sm = mt_marks(sh, tid, hm, len, &bytes, &last_end);
    uint32_t dm = 0;
    if constexpr (GATHER)
        dm = a.records ? bzf_eq_mask16(own.x, own.y, own.z, own.w, m.delim()) & bzf_range_mask16(p0, w.d_lo, w.n) : 0u;
    mt_sum_put(sh, tid, (uint32_t)__popc(sm), bytes, (uint32_t)__popc(dm));
    match_sums(sh, tid);
    if constexpr (!GATHER) {
        mt_last_end(sh, tid, sm, last_end);
        __syncthreads();
        if (tid == 0) a.cnt[blockIdx.x] = MtCount{mt_s_cnt(mt_sum_all(sh)), mt_s_bytes(mt_sum_all(sh)), sh.last_end, 0};
    } else {
        uint8_t *comp = reinterpret_cast<uint8_t *>(sh.y); // (the marks are made: nobody reads y any more)
        const MtBase base = a.base[blockIdx.x];
        mt_gather(m, msh, comp, sm, len, dm, mt_sum_excl(sh, tid), tile + tid * BZF_ITEMS, p0, w, a.records, base, a.win.out_base, a.out != nullptr, a.ent);
        if (!a.out) return;
        __syncthreads();
        mt_store(comp, tid, a.out + a.win.out_base + base.bytes, want);
    }
}

// The sums in front of every tile, one workgroup; the window's totals.
__global__ void __launch_bounds__(BZF_THREADS) match_sum(const MtCount *cnt, uint32_t tiles, MtBase *base, uint64_t *totals)
{
    __shared__ MtSumShared sh;
    const uint32_t tid = threadIdx.x;
    mt_sum_a(sh, tid, cnt, tiles);
    __syncthreads();
    if (tid == 0) mt_sum_b(sh, totals);
    __syncthreads();
    mt_sum_c(sh, tid, cnt, tiles, base);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
// The passes over the window of d (16-byte aligned; w.n bytes lie there, and the aligned word that holds the last of them).  One
// wait, for the window's totals; bytes and entries follow the stream and are there after the call's last wait.
static int match_window_run(bzh_ctx *ctx, MatchSink &s, const uint8_t *d, const MtWindow &mw, uint64_t bytes, bool last)
{
    hipStream_t st = ctx->stream;
    bzh_match_stats &ms = ctx->mtstats;
    const BzfWindow &w = mw.w;
    const BzfPick pick{mw.lim, w.n, 0 - w.off_base, BZR_LOOK_EDGE}; // (output offset 0 lies at position 0 - off_base: the text's edge stands in front of it)
    uint32_t tiles;
    BZH_TRY(scan_tiles(ctx, "match", w.n, &ms.windows, &ms.tiles, &tiles));
    uint64_t totals[MT_TOTALS] = {0, 0, 0, 0, 0, 0, 0};
    if (s.walk.runs(mw, s.records)) {
        MfArgs a{d, mw, s.records ? 1u : 0u, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        uint8_t *summ = nullptr;
        uint64_t *d_tot = nullptr;
        BZH_TRY(reserve_cut(ctx, ctx->match_tab, "the match tables", grow_mib, [&](Carver &c) {
            c.put(a.lens, (size_t)tiles * BZF_TILE), c.put(a.base, tiles), c.put(d_tot, MT_TOTALS), c.put(a.tile, tiles), c.put(a.cnt, tiles);
            c.put(a.hits, (size_t)tiles * BZF_THREADS), c.put(a.map, (size_t)tiles * 256u), c.put(summ, 256u * 256u);
        }));
        pick_matcher(s.pat, s.set, s.delim, pick, [&](const auto &m) { match_tiles<<<dim3(tiles), BZF_THREADS, 0, st>>>(a, m); });
        match_scan<<<dim3(1), BZF_THREADS, 0, st>>>(a.tile, a.map, tiles, a.base, summ, d_tot);
        match_select<false><<<dim3(tiles), BZF_THREADS, 0, st>>>(a, MtNoMatcher{});
        match_sum<<<dim3(1), BZF_THREADS, 0, st>>>(a.cnt, tiles, a.base, d_tot);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(totals, d_tot, sizeof totals, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, bzh_stream_wait(st));
        if (s.walk.gather(totals)) {
            a.out = s.walk.want_out ? s.d_out : nullptr;
            if (s.walk.want_ent) {
                BZH_TRY(ctx->match_ent.reserve(ctx, (size_t)totals[MT_T_SEL] * sizeof(MtEntry), "the match entries", grow_mib));
                a.ent = ctx->match_ent.as<MtEntry>();
            }
            pick_matcher(s.pat, s.set, s.delim, pick, [&](const auto &m) { match_select<true><<<dim3(tiles), BZF_THREADS, 0, st>>>(a, m); });
            HIP_TRY(ctx, hipGetLastError());
            if (a.ent)
                HIP_TRY(ctx, hipMemcpyAsync(s.ent + w.rank_base, a.ent, (size_t)totals[MT_T_SEL] * sizeof(MtEntry), hipMemcpyDeviceToHost, st));
        }
    }
    s.walk.advance(mw, bytes, totals, last);
    ms.matches = s.walk.sel, ms.out_bytes = s.walk.out_bytes, ms.candidates = s.walk.candidates;
    ms.entered_tiles = s.walk.entered, ms.open_tiles = s.walk.open, ms.carry_peak = s.walk.carry_peak;
    return BZH_OK;
}

int MatchSink::room(bzh_ctx *ctx, uint64_t bytes, uint8_t **d_stage)
{
    return scan_room(ctx, "the match staging", walk.walk.carry, bytes, &ctx->mtstats.staging_peak, d_stage, &at);
}

// The passes, and the window's tail is kept as the carry.
int MatchSink::window(bzh_ctx *ctx, uint64_t bytes)
{
    const uint8_t *base = ctx->search_ws.p;
    const MtWindow mw = walk.window(at, bytes, false);
    const uint64_t keep = walk.carry_after(bytes);
    if (keep) { // [n - keep, n): read before the passes' wait, written where no pass looks
        BZH_TRY(ctx->scan_carry.reserve(ctx, BZF_MAX_PATTERN + 16, "the match carry")); // (with assertions up to 257 bytes)
        HIP_TRY(ctx, hipMemcpyAsync(ctx->scan_carry, base + mw.w.n - keep, (size_t)keep, hipMemcpyDeviceToDevice, ctx->stream));
    }
    return match_window_run(ctx, *this, base, mw, bytes, false);
}

// Decoded bytes that already lie in HBM: one window, no staging, no carry.
int MatchSink::raw(bzh_ctx *ctx, const uint8_t *d_raw, size_t n)
{
    return match_window_run(ctx, *this, d_raw, walk.window(0, n, true), n, true);
}

// Behind the last window: the starts held back are processed where they lie, in the carry -- a window without new bytes, its
// text the carry, every delimiter of which has been counted.
int MatchSink::finish(bzh_ctx *ctx)
{
    if (!walk.walk.carry) return BZH_OK;
    return match_window_run(ctx, *this, ctx->scan_carry, walk.window(walk.walk.carry, 0, true), 0, true);
}

// Bytes and entries have followed the stream to the caller's arrays; the counts, and whether the rooms sufficed.
int MatchSink::report(bzh_ctx *ctx, size_t *nmatches, uint64_t *out_total)
{
    *nmatches = (size_t)walk.sel;
    *out_total = walk.out_bytes;
    if (walk.overflow()) {
        bzh_set_error(ctx, "match: %llu matches of %llu bytes, room for %llu and %llu", (unsigned long long)walk.sel,
                      (unsigned long long)walk.out_bytes, (unsigned long long)walk.max, (unsigned long long)walk.cap);
        return BZH_E_CAP;
    }
    return BZH_OK;
}
