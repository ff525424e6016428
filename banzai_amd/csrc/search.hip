// search.hip -- every occurrence of a byte string in decoded bytes that lie in HBM (bzh_search*): the kernel, the two passes over
// one window, and the staging buffer the decoders expand into (the windows and the carry: search_plan.h; what one thread does:
// search_core.h).  The bytes never leave the device: what comes back is a word a window, and the hits.
#include "common.h"
#include "search_core.h"

static_assert(BZF_MAX_PATTERN == BZH_SEARCH_MAX_PATTERN, "search_core.h and bzhip.h name the same bound");
static_assert(BZF_FRONT % 16 == 0 && BZF_FRONT >= BZF_MAX_PATTERN, "a window begins aligned, its carry in front of it");
static_assert(sizeof(bzh_hit) == 16, "a hit is two words");

struct SfPat { // the pattern, by value in the kernel's arguments
    uint32_t w[BZF_MAX_PATTERN / 4];
};

struct SfArgs {
    const uint8_t *d; // 16-byte aligned
    BzfWindow win;
    uint32_t plen, delim, records;
    uint32_t head, hmask;          // the filter's word and mask (search_core.h)
    uint32_t *thits, *tdel;        // [tiles] pass one: hits and delimiters of every tile
    const uint64_t *hbase, *dbase; // [tiles] search_scan: those in front of every tile
    bzh_hit *out;                  // the window's hit slots [0, win.emit)
};

// A thread's 16 bytes at position p0 of d[0, n).  Inside the text: one aligned 16-byte load.  At its end: the aligned 4-byte words
// that begin in front of n, zeros behind them -- no read goes past the word that holds byte n - 1.
__device__ __forceinline__ uint4 sf_load16(const uint8_t *d, uint64_t n, uint64_t p0)
{
    if (p0 + 16 <= n) return *reinterpret_cast<const uint4 *>(d + p0);
    uint4 v;
    v.x = p0 < n ? *reinterpret_cast<const uint32_t *>(d + p0) : 0u;
    v.y = p0 + 4 < n ? *reinterpret_cast<const uint32_t *>(d + p0 + 4) : 0u;
    v.z = p0 + 8 < n ? *reinterpret_cast<const uint32_t *>(d + p0 + 8) : 0u;
    v.w = p0 + 12 < n ? *reinterpret_cast<const uint32_t *>(d + p0 + 12) : 0u;
    return v;
}

// One workgroup a tile of 4,096 positions, 16 a thread.  The tile and the halo behind it are staged in LDS, the pattern too (every
// lane reads the same byte of it).  EMIT false: the tile's hits and delimiters, reduced over the workgroup, a plain store each -- no
// atomics; search_scan sums the tiles.  EMIT true: the same tests again, in tiles that hold a hit in front of the caller's bound,
// and every hit whose rank in the window is below win.emit stores itself at its rank: the output ascends, and "the first max" costs
// nothing.  Stores: the tile's two words, or hit slots below win.emit.
template <bool EMIT>
__global__ void __launch_bounds__(BZF_THREADS) search_tiles(SfArgs a, SfPat p)
{
    __shared__ __attribute__((aligned(16))) uint8_t tile[BZF_TILE + BZF_MAX_PATTERN];
    __shared__ __attribute__((aligned(4))) uint8_t pat[BZF_MAX_PATTERN];
    __shared__ uint32_t lds[8];
    const uint32_t tid = threadIdx.x;
    if (EMIT && (a.thits[blockIdx.x] == 0 || a.hbase[blockIdx.x] >= a.win.emit)) return; // (the same for every thread)
    const uint64_t n = a.win.n, t0 = (uint64_t)blockIdx.x * BZF_TILE, p0 = t0 + tid * BZF_ITEMS;
    if (tid < BZF_MAX_PATTERN / 4) reinterpret_cast<uint32_t *>(pat)[tid] = p.w[tid];
    const uint4 own = sf_load16(a.d, n, p0);
    *reinterpret_cast<uint4 *>(tile + tid * BZF_ITEMS) = own;
    if (tid * BZF_ITEMS < a.plen - 1) // the halo: the head of the next tile, as far as a match that starts in this one can reach
        *reinterpret_cast<uint4 *>(tile + BZF_TILE + tid * BZF_ITEMS) = sf_load16(a.d, n, t0 + BZF_TILE + tid * BZF_ITEMS);
    __syncthreads();
    const uint32_t next = *reinterpret_cast<const uint32_t *>(tile + tid * BZF_ITEMS + BZF_ITEMS); // (thread 255: the halo's first word, or what lies there)
    const uint32_t dm = a.records ? bzf_eq_mask16(own.x, own.y, own.z, own.w, a.delim) & bzf_range_mask16(p0, a.win.d_lo, n) : 0u;
    uint32_t cand = bzf_filter16(own.x, own.y, own.z, own.w, next, bzf_range_mask16(p0, a.win.s_lo, a.win.s_hi), a.head, a.hmask);
    uint32_t hm = cand;
    if (a.plen > 4) {
        hm = 0;
        while (cand) {
            const uint32_t k = (uint32_t)__ffs((int)cand) - 1u;
            cand &= cand - 1u;
            if (bzf_verify(tile + tid * BZF_ITEMS + k, pat, a.plen)) hm |= 1u << k;
        }
    }
    const uint32_t nh = (uint32_t)__popc(hm), nd = (uint32_t)__popc(dm);
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
        if (rank < a.win.emit) {
            const uint64_t pos = p0 + k;
            uint64_t rec = 0;
            if (a.records) {
                if (pos >= a.win.d_lo) {
                    rec = a.win.rec_base + a.dbase[blockIdx.x] + d0 + bzf_delims_before(dm, k);
                } else { // a start in the carry: the delimiters between it and d_lo were counted by the window before
                    const uint32_t gap = (uint32_t)min(a.win.d_lo - pos, (uint64_t)(BZF_MAX_PATTERN - 1)); // (the halo holds them)
                    uint32_t c = 0;
                    for (uint32_t j = 0; j < gap; j++) c += tile[tid * BZF_ITEMS + k + j] == a.delim;
                    rec = a.win.rec_base - c;
                }
            }
            a.out[rank] = bzh_hit{a.win.off_base + pos, rec};
        }
        rank++;
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

// ---- host side ---------------------------------------------------------------------------------------------------
int search_job(SearchJob &job, const uint8_t *pat, size_t plen, unsigned flags, uint8_t delim, bzh_hit *hits, size_t max)
{
    memset(&job, 0, sizeof job);
    memcpy(job.pat, pat, plen);
    job.plen = (uint32_t)plen;
    job.delim = delim;
    job.records = (flags & BZH_SEARCH_RECORDS) != 0;
    job.hits = hits;
    job.max = max;
    return BZH_OK;
}

// The two passes over the window w of d (16-byte aligned; w.n bytes lie there, and the aligned word that holds the last of them).
// One wait, for the window's two totals; the hits follow the stream to the caller's array and are there after the call's last wait.
int search_window_run(bzh_ctx *ctx, const SearchJob &job, BzfWalk &walk, const uint8_t *d, BzfWindow w, uint64_t bytes)
{
    hipStream_t st = ctx->stream;
    bzh_search_stats &ss = ctx->sstats;
    const uint64_t tiles64 = (w.n + BZF_TILE - 1) / BZF_TILE;
    if (tiles64 > 0x7FFFFFFFull) {
        bzh_set_error(ctx, "search: a window of %llu bytes is beyond one launch", (unsigned long long)w.n);
        return BZH_E_ARG;
    }
    const uint32_t tiles = (uint32_t)tiles64;
    ss.windows++;
    ss.tiles += tiles;
    uint64_t totals[2] = {0, 0};
    if (tiles && (w.s_hi > w.s_lo || job.records)) {
        uint32_t *thits = nullptr, *tdel = nullptr;
        uint64_t *hbase = nullptr, *dbase = nullptr, *d_tot = nullptr;
        BZH_TRY(reserve_cut(ctx, ctx->search_tab, "the search's tile tables", grow_mib, [&](Carver &c) {
            c.put(hbase, tiles), c.put(dbase, tiles), c.put(d_tot, 2), c.put(thits, tiles), c.put(tdel, tiles);
        }));
        SfPat p;
        memcpy(p.w, job.pat, sizeof p.w);
        SfArgs a{d, w, job.plen, job.delim, job.records ? 1u : 0u, bzf_head_word(job.pat, job.plen), bzf_head_mask(job.plen), thits, tdel,
                 hbase, dbase, nullptr};
        search_tiles<false><<<dim3(tiles), BZF_THREADS, 0, st>>>(a, p);
        search_scan<<<dim3(1), BZF_THREADS, 0, st>>>(thits, tdel, tiles, hbase, dbase, d_tot);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(totals, d_tot, sizeof totals, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, bzh_stream_wait(st));
        const uint64_t emit = walk.emit(totals[0]);
        if (emit) {
            BZH_TRY(ctx->search_out.reserve(ctx, (size_t)emit * sizeof(bzh_hit), "the search's hits", grow_mib));
            a.win.emit = emit;
            a.out = ctx->search_out.as<bzh_hit>();
            search_tiles<true><<<dim3(tiles), BZF_THREADS, 0, st>>>(a, p);
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipMemcpyAsync(job.hits + walk.rank, a.out, (size_t)emit * sizeof(bzh_hit), hipMemcpyDeviceToHost, st));
        }
    }
    walk.advance(bytes, totals[0], totals[1]);
    ss.hits = walk.rank;
    return BZH_OK;
}

// The staging buffer for a window of `bytes` decoded bytes: grown to it (whole blocks, at least one, so a block above the target
// grows it), the carry put in front of BZF_FRONT.  *d_stage = its base; the decoders expand at *d_stage + BZF_FRONT.
int search_sink_room(bzh_ctx *ctx, SearchSink &sink, uint64_t bytes, uint8_t **d_stage)
{
    if (sink.grep) return grep_sink_room(ctx, *sink.grep, bytes, d_stage);
    uint8_t *base = nullptr;
    BZH_TRY(reserve_cut(ctx, ctx->search_ws, "the search's staging", grow_mib, [&](Carver &c) { c.put(base, (size_t)(BZF_FRONT + bytes + 16)); }));
    ctx->sstats.staging_peak = std::max<uint64_t>(ctx->sstats.staging_peak, ctx->search_ws.cap);
    const uint64_t carry = sink.walk.carry;
    if (carry) // (kept apart between two windows: the staging buffer may have moved)
        HIP_TRY(ctx, hipMemcpyAsync(base + BZF_FRONT - carry, ctx->search_carry, (size_t)carry, hipMemcpyDeviceToDevice, ctx->stream));
    *d_stage = base;
    return BZH_OK;
}

// The window search_sink_room made room for has been expanded and verified: the two passes, then its tail is kept as the carry.
int search_sink_window(bzh_ctx *ctx, SearchSink &sink, uint64_t bytes)
{
    if (sink.grep) return grep_sink_window(ctx, *sink.grep, bytes);
    const uint8_t *base = ctx->search_ws.p;
    const BzfWindow w = sink.walk.window(bytes);
    const uint64_t keep = sink.walk.carry_after(bytes);
    if (keep) { // [n - keep, n): read before the passes' wait, written where no pass looks
        BZH_TRY(ctx->search_carry.reserve(ctx, BZF_MAX_PATTERN, "the search's carry"));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->search_carry, base + w.n - keep, (size_t)keep, hipMemcpyDeviceToDevice, ctx->stream));
    }
    return search_window_run(ctx, sink.job, sink.walk, base, w, bytes);
}

// Decoded bytes that already lie in HBM: one window, no staging, no carry.
int search_raw_run(bzh_ctx *ctx, SearchSink &sink, const uint8_t *d_raw, size_t n)
{
    sink.walk.begin(sink.job.plen, 0, sink.job.max, 0, n, 0, 0);
    return search_window_run(ctx, sink.job, sink.walk, d_raw, sink.walk.window(n), n);
}
