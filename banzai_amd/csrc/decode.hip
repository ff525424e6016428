// decode.hip -- the bzip2 DECODER (bzh_decode*, include/bzhip.h).  The reference has none (README.md:9); the format is the
// one it writes (lib/lib.rs:18-70, lib/huffman.rs:464-572) and libbz2 reads.
//
//   scan     : every occurrence of the block and the footer magic, at any bit alignment     (decode_scan_kernel)
//   entropy  : one wavefront per candidate: header, tables, symbols -> last column           (decode_block_kernel, decode_core.h)
//   chain    : the host walks from block end to block start; candidates inside a payload drop out
//   unbwt    : the inverse transform of the batch                                            (unbwt_run, bwt.hip)
//   unrle    : inverse RLE1 -- roles by a scan of state maps, sizes, then the expansion      (unrle_maps / unrle_walk; one tile
//              front, ur_enter / ur_place, under every unrle_* kernel of this file)
//   crc      : block CRCs over the output ranges (rle1.hip), folded per stream on the host
// Random access (bzh_decode_index*, bzh_decode_range*): the index is the chain walk with no output, every block's CRC taken
// from the bytes behind the inverse BWT (unrle_crc); a range decodes the blocks its index entries name, no scan and no walk,
// and clips the blocks at its two edges to the range (unrle_walk_win).
// Sync points (bzh_decode_index_sync*, bzh_decode_range_sync*): the index build also writes the entropy stage's state down every
// `interval` groups (decode_block_sync_kernel); a range then parses each touched block's header once (decode_header_kernel) and
// decodes every segment, from point to point, in a wavefront of its own (decode_segment_kernel).
// Records (bzh_decode_index_records*, bzh_decode_records*, bzh_count_records_device): the index build also counts every block's
// delimiter bytes where it folds the CRC (unrle_count); a read by record number decodes the blocks the table names, finds the
// boundary delimiters on the device (unrle_select) and emits the records' bytes through the pieces of the range decode.
// Every read by index -- one range, many ranges, records -- takes its batches through one front (IndexedFront: the entropy stage
// of a list of entries, every block checked against its entry, back_sizes) and differs in what it asks of back_emit behind it.
#include <algorithm>
#include <type_traits>
#include <vector>

#include "common.h"
#include "crc_gf.h"
#include "decode_core.h"
#include "decode_plan.h"
#include "decode_many_plan.h"
#include "decode_records_plan.h"
#include "decode_recover_plan.h"
#include "decode_stream_plan.h"

// ---- scan ------------------------------------------------------------------------------------------------------
// 16 start bytes a lane, all 8 shifts of each against both 48-bit magics.  Hits are rare: an atomic append (the host sorts).
constexpr uint32_t SCAN_THREADS = 256, SCAN_BYTES = 16;

__global__ void __launch_bounds__(SCAN_THREADS) decode_scan_kernel(const uint8_t *in, uint64_t n, uint64_t *list, uint32_t cap, uint32_t *count)
{
    const uint64_t i0 = ((uint64_t)blockIdx.x * SCAN_THREADS + threadIdx.x) * SCAN_BYTES;
    if (i0 >= n) return;
    uint64_t q[3]; // bytes i0 .. i0+23, big-endian words, zero behind the input
    if (i0 + 24 <= n) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            uint64_t v;
            __builtin_memcpy(&v, in + i0 + 8 * k, 8);
            q[k] = __builtin_bswap64(v);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            uint64_t v = 0;
            for (int j = 0; j < 8; j++) {
                const uint64_t at = i0 + 8 * k + j;
                v = (v << 8) | (at < n ? (uint64_t)in[at] : 0ull);
            }
            q[k] = v;
        }
    }
    const uint64_t nbits = n * 8;
#pragma unroll
    for (int k = 0; k < (int)SCAN_BYTES; k++) {
        const uint64_t a = q[k >> 3], b = q[(k >> 3) + 1];
        const int sh = 8 * (k & 7);
        const uint64_t w = sh ? (a << sh) | (b >> (64 - sh)) : a; // the 8 bytes from start byte k
#pragma unroll
        for (int s = 0; s < 8; s++) {
            const uint64_t v = (w << s) >> 16;
            const bool blk = v == BZD_BLOCK_MAGIC, ftr = v == BZD_FOOTER_MAGIC;
            if (blk || ftr) {
                const uint64_t bitpos = (i0 + k) * 8 + s;
                if (bitpos + 48 <= nbits) { // (the footer magic ends in zero bits: not past the end of the input)
                    const uint32_t at = atomicAdd(count, 1u);
                    if (at < cap) list[at] = bitpos << 1 | (ftr ? 1ull : 0ull);
                }
            }
        }
    }
}

// ---- entropy stage ---------------------------------------------------------------------------------------------
// One wavefront per candidate.  A slot whose candidate did not decode is left as a one-byte block, so that the inverse
// transform of the batch has nothing to trip over.
__global__ void __launch_bounds__(64) decode_block_kernel(const uint8_t *in, uint64_t n, const uint64_t *cand, Batch bt, BzdResult *res,
                                                           uint32_t block_max)
{
    __shared__ BzdWork w;
    const uint32_t b = blockIdx.x;
    const uint64_t c0 = cand[b];
    const uint64_t c = (uint64_t)BZD_UNI((uint32_t)c0) | (uint64_t)BZD_UNI((uint32_t)(c0 >> 32)) << 32;
    uint8_t *L = bt.bwt + (size_t)b * bt.S;
    BzdResult r;
    if (c & 1ull)
        bzd_parse_footer(in, n, c >> 1, r);
    else
        bzd_decode_block(w, in, n, c >> 1, block_max, L, r);
    if (threadIdx.x == 0) {
        const bool ok = !(c & 1ull) && r.kind == BZD_OK;
        res[b] = r;
        bt.n[b] = ok ? r.nblock : 1u;
        bt.ptr[b] = ok ? r.origptr : 0u;
        if (!ok) L[0] = 0;
    }
}

// ---- sync points: recording --------------------------------------------------------------------------------------------
// The recorder of the index build: the points of a candidate go to its slot's region, `cap` of them at most.
struct SyncRecorder {
    static constexpr bool ON = true;
    uint32_t interval;
    bzh_sync_point *pts;
    uint32_t cap, count;
    __host__ __device__ __forceinline__ void point(uint64_t pos, uint32_t gi, uint32_t nblock, uint32_t run, uint32_t run_weight, const uint8_t *mtf)
    {
        if (count >= cap) return;
        bzh_sync_point *p = pts + count;
        if (BZD_LANE == 0) {
            p->bit_pos = pos;
            p->entry = 0; // (the host numbers the entries: the chain decides which candidates are blocks)
            p->group = gi;
            p->out_pos = nblock;
            p->run = run;
            p->run_weight = run_weight;
            p->reserved = 0;
        }
        for (uint32_t i = BZD_LANE; i < 256; i += BZD_LANES) p->mtf[i] = mtf[i];
        count++;
    }
};

// decode_block_kernel with the recorder: one wavefront per candidate, the same bounds.  cnt[b] = points of slot b.
__global__ void __launch_bounds__(64) decode_block_sync_kernel(const uint8_t *in, uint64_t n, const uint64_t *cand, Batch bt, BzdResult *res,
                                                                uint32_t block_max, uint32_t interval, bzh_sync_point *pts, uint32_t cap,
                                                                uint32_t *cnt)
{
    __shared__ BzdWork w;
    const uint32_t b = blockIdx.x;
    const uint64_t c0 = cand[b];
    const uint64_t c = (uint64_t)BZD_UNI((uint32_t)c0) | (uint64_t)BZD_UNI((uint32_t)(c0 >> 32)) << 32;
    uint8_t *L = bt.bwt + (size_t)b * bt.S;
    BzdResult r;
    SyncRecorder rec{interval, pts + (size_t)b * cap, cap, 0};
    if (c & 1ull)
        bzd_parse_footer(in, n, c >> 1, r);
    else
        bzd_decode_block_rec(w, in, n, c >> 1, block_max, L, r, rec);
    if (threadIdx.x == 0) {
        const bool ok = !(c & 1ull) && r.kind == BZD_OK;
        res[b] = r;
        bt.n[b] = ok ? r.nblock : 1u;
        bt.ptr[b] = ok ? r.origptr : 0u;
        cnt[b] = ok ? rec.count : 0u;
        if (!ok) L[0] = 0;
    }
}

// ---- sync points: the segmented entropy stage ------------------------------------------------------------------------------
// What decode_header_kernel leaves of a block for its segments (global memory).
struct BzdHead {
    uint16_t lut[6][1u << BZD_LUT_BITS];
    int32_t limit[6][BZD_MAX_LEN + 2], base[6][BZD_MAX_LEN + 2];
    uint16_t perm[6][258];
    uint32_t minlen[6], maxlen[6];
    uint32_t nin, nsel, ngroups, origptr;
    uint64_t first_bit; // of the first code
    uint8_t mtf[256];   // the initial MTF list
    uint8_t sel[BZD_MAX_SEL + 1];
};

// The tables a segment keeps in LDS: 16,744 bytes a wavefront (BzdWork: 51 KB).  The selectors stay in global memory -- one
// wave-uniform byte load per 50 symbols -- and the code lengths are not needed behind the header.
struct BzdSegWork {
    uint16_t lut[6][1u << BZD_LUT_BITS];
    int32_t limit[6][BZD_MAX_LEN + 2], base[6][BZD_MAX_LEN + 2];
    uint16_t perm[6][258];
    uint32_t minlen[6], maxlen[6];
    uint8_t mtf[256];
};
static_assert(sizeof(BzdSegWork) <= 17 * 1024, "the segment kernel's LDS budget");

template <class D, class S>
__device__ __forceinline__ void seg_copy_tables(D &d, const S &s, uint32_t ngroups, uint32_t alpha)
{
    const uint32_t lane = threadIdx.x;
    for (uint32_t t = 0; t < ngroups; t++) {
        const uint32_t *ls = reinterpret_cast<const uint32_t *>(s.lut[t]);
        uint32_t *ld = reinterpret_cast<uint32_t *>(d.lut[t]);
        for (uint32_t i = lane; i < (1u << BZD_LUT_BITS) / 2; i += 64) ld[i] = ls[i];
        for (uint32_t i = lane; i < BZD_MAX_LEN + 2; i += 64) {
            d.limit[t][i] = s.limit[t][i];
            d.base[t][i] = s.base[t][i];
        }
        for (uint32_t i = lane; i < alpha; i += 64) d.perm[t][i] = s.perm[t][i];
    }
    if (lane < ngroups) {
        d.minlen[lane] = s.minlen[lane];
        d.maxlen[lane] = s.maxlen[lane];
    }
}

// One wavefront per touched block: the header, parsed once.  res[b]: kind / errpos / crc / origptr (end_bit and nblock come from
// the block's last segment).
__global__ void __launch_bounds__(64) decode_header_kernel(const uint8_t *in, uint64_t n, const uint64_t *cand, BzdHead *heads, BzdResult *res)
{
    __shared__ BzdWork w;
    const uint32_t b = blockIdx.x, lane = threadIdx.x;
    const uint64_t c0 = cand[b];
    const uint64_t c = (uint64_t)BZD_UNI((uint32_t)c0) | (uint64_t)BZD_UNI((uint32_t)(c0 >> 32)) << 32;
    BzdResult r;
    r.kind = BZD_OK;
    r.crc = 0;
    r.errpos = 0;
    r.end_bit = 0;
    r.nblock = 0;
    r.origptr = 0;
    r.follow = 0;
    r.pad = 0;
    BzdBits rd;
    bzd_seek(rd, in, n, (c >> 1) + 48);
    BzdHdr h;
    if (bzd_parse_header(w, rd, r, h)) {
        BzdHead &H = heads[b];
        seg_copy_tables(H, w, h.ngroups, h.nin + 2);
        for (uint32_t i = lane; i < 256; i += 64) H.mtf[i] = w.mtf[i];
        for (uint32_t i = lane; i < h.nsel; i += 64) H.sel[i] = w.sel[i];
        if (lane == 0) {
            H.nin = h.nin;
            H.nsel = h.nsel;
            H.ngroups = h.ngroups;
            H.origptr = r.origptr;
            H.first_bit = rd.pos;
        }
    }
    if (lane == 0) res[b] = r;
}

__device__ __forceinline__ BzdSyncState seg_state(const bzh_sync_point *p, uint64_t bit_base)
{
    BzdSyncState s;
    const uint64_t pos = p->bit_pos - bit_base; // (the host has checked: inside its entry, which lies inside the buffer)
    s.bit_pos = (uint64_t)BZD_UNI((uint32_t)pos) | (uint64_t)BZD_UNI((uint32_t)(pos >> 32)) << 32;
    s.group = BZD_UNI(p->group);
    s.out_pos = BZD_UNI(p->out_pos);
    s.run = BZD_UNI(p->run);
    s.run_weight = BZD_UNI(p->run_weight);
    s.mtf = p->mtf;
    return s;
}

// One wavefront per segment of every touched block of the batch.  It writes bytes [from.out_pos, to.out_pos) of its block's last
// column and nothing else of it; the block's last segment also leaves the block's size and origPtr for the inverse transform.
__global__ void __launch_bounds__(64) decode_segment_kernel(const uint8_t *in, uint64_t n, uint64_t bit_base, const BzdHead *heads,
                                                             const bzh_sync_point *pts, const SegDesc *segs, Batch bt, BzdResult *res,
                                                             BzdSegResult *sres)
{
    __shared__ BzdSegWork w;
    const uint32_t g = blockIdx.x;
    const uint32_t slot = BZD_UNI(segs[g].slot), block_max = BZD_UNI(segs[g].block_max);
    const int32_t from_i = (int32_t)BZD_UNI(segs[g].from), to_i = (int32_t)BZD_UNI(segs[g].to);
    BzdSegResult sr;
    sr.kind = BZD_UNI(res[slot].kind);
    sr.miss = BZD_SEG_OK;
    sr.errpos = 0;
    sr.end_bit = 0;
    sr.nblock = 0;
    sr.pad = 0;
    if (sr.kind == BZD_OK) { // (a header that did not parse left no tables: the host reports it for the block)
        const BzdHead &H = heads[slot];
        const uint32_t nin = BZD_UNI(H.nin), nsel = BZD_UNI(H.nsel), ngroups = BZD_UNI(H.ngroups), origptr = BZD_UNI(H.origptr);
        seg_copy_tables(w, H, ngroups, nin + 2);
        BzdSyncState from, to = {};
        if (from_i >= 0) {
            from = seg_state(pts + from_i, bit_base);
        } else {
            const uint64_t fb = H.first_bit;
            from.bit_pos = (uint64_t)BZD_UNI((uint32_t)fb) | (uint64_t)BZD_UNI((uint32_t)(fb >> 32)) << 32;
            from.group = 0;
            from.out_pos = 0;
            from.run = 0;
            from.run_weight = 1;
            from.mtf = H.mtf;
        }
        if (to_i >= 0) to = seg_state(pts + to_i, bit_base);
        uint8_t *L = bt.bwt + (size_t)slot * bt.S;
        // (from.out_pos <= block_max <= S is checked inside before anything is stored)
        bzd_decode_segment(w, H.sel, in, n, nin, nsel, origptr, from, to_i >= 0, to, block_max, L + from.out_pos, sr);
        if (threadIdx.x == 0 && to_i < 0 && sr.kind == BZD_OK && sr.miss == BZD_SEG_OK) {
            bt.n[slot] = sr.nblock;
            bt.ptr[slot] = origptr;
        }
    }
    if (threadIdx.x == 0) sres[g] = sr;
}

// ---- inverse RLE1 ----------------------------------------------------------------------------------------------
// A tile = 4096 bytes of a block, 16 a thread.  unrle_maps: the tile's state map.  unrle_walk<false>: the tile's entry state
// (the maps of the tiles before it, composed) and its output bytes; <true>: the expansion, at offsets the host has summed.
// Every unrle_* kernel behind unrle_maps enters its tile through one front -- ur_enter: the load, the scan of the threads' maps,
// the thread's state; ur_place on top of it for the three that store bytes: the thread's first position and the one bound on
// every position -- and what a thread does with its 16 bytes is decode_core.h's text (bzd_ur_*), which the host harnesses run too.
constexpr uint32_t UR_THREADS = 256, UR_ITEMS = 16, UR_TILE = UR_THREADS * UR_ITEMS, UR_STAGE = 8192;

struct UrArgs {
    const uint8_t *x;      // [B][S] the blocks (output of the inverse transform)
    const uint32_t *n;     // [B]
    const uint32_t *slots; // [K] batch slots of the blocks on the chain
    uint32_t S, T;         // T = tiles per block stride
    uint32_t *tmap, *tout, *tstate; // [B][T]
    uint32_t *endstate;    // [B] state behind the block's last byte
    const uint32_t *toff;  // [B][T] output offset of the tile inside its block
    const uint64_t *obase; // [K] output offset of the block
    uint8_t *out;
};

struct UrBytes {
    uint32_t w[4];
    uint32_t cnt;  // bytes of this thread inside the block
    uint32_t prev; // the byte before them (256: none)
};

__device__ __forceinline__ UrBytes ur_load(const uint8_t *x, uint32_t n, uint32_t i0)
{
    UrBytes u;
    u.cnt = i0 < n ? min(UR_ITEMS, n - i0) : 0u;
    u.prev = 256;
    u.w[0] = u.w[1] = u.w[2] = u.w[3] = 0;
    if (u.cnt) { // (16-byte aligned, and inside the block's stride: S is a multiple of the tile)
        const uint4 v = *reinterpret_cast<const uint4 *>(x + i0);
        u.w[0] = v.x;
        u.w[1] = v.y;
        u.w[2] = v.z;
        u.w[3] = v.w;
        if (i0) u.prev = x[i0 - 1];
    }
    return u;
}

// exclusive scan of state maps over the workgroup (composition in thread order); *total = all of them.  lds: 4 words.
__device__ __forceinline__ uint32_t ur_scan(uint32_t m, uint32_t *lds, uint32_t *total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = m;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)inc, d, 64);
        if (lane >= (uint32_t)d) inc = bzd_rl_compose(t, inc);
    }
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    uint32_t carry = BZD_RL_ID, tot = BZD_RL_ID;
    for (uint32_t k = 0; k < UR_THREADS / 64; k++) {
        if (k < wave) carry = bzd_rl_compose(carry, lds[k]);
        tot = bzd_rl_compose(tot, lds[k]);
    }
    uint32_t ex = (uint32_t)__shfl_up((int)inc, 1, 64);
    if (lane == 0) ex = BZD_RL_ID;
    __syncthreads();
    *total = tot;
    return bzd_rl_compose(carry, ex);
}

static_assert(UR_ITEMS == BZD_UR_ITEMS, "decode_core.h walks the same 16 bytes a thread");

// The tile front of every kernel that is handed its entry state.  Thread threadIdx.x of tile t of slot b, a block of n bytes:
// its 16 bytes, the scan of the threads' maps, *s = the state the thread's first byte is met in.  Slot, tile and n are the
// caller's (a grid cell, or a query that the caller has bounded), and every read lies below n inside the slot's stride.
__device__ __forceinline__ UrBytes ur_enter(const UrArgs &a, uint32_t n, uint32_t b, uint32_t t, uint32_t entry, uint32_t *lds, uint32_t *s)
{
    const UrBytes u = ur_load(a.x + (size_t)b * a.S, n, t * UR_TILE + threadIdx.x * UR_ITEMS);
    uint32_t total;
    const uint32_t ex = ur_scan(bzd_ur_map(u.w, u.cnt, u.prev), lds, &total);
    *s = bzd_rl_apply(ex, entry);
    return u;
}

// The front of the kernels that place bytes: ur_enter, then where this thread's bytes begin inside the tile's expansion.
// `lim` bounds every position a caller stores at, in LDS or in global memory: it is the smaller of tile_total -- a.tout, what
// unrle_walk<false> summed over these same bytes and the host laid the output out by, known before anything is loaded and the
// one that decides staged or not -- and this walk's own sum.  The two are equal by construction; clipping to both keeps every
// position below both without relying on that.  (unrle_walk<false>, which makes a.tout, passes no bound: lim is its sum.)
struct UrPlace {
    UrBytes u;
    uint32_t s, s_end; // the state the thread's bytes are entered in, and the one behind them
    uint32_t o0, lim;
};

__device__ __forceinline__ UrPlace ur_place(const UrArgs &a, uint32_t n, uint32_t b, uint32_t t, uint32_t entry, uint32_t tile_total, uint32_t *lds)
{
    UrPlace p;
    p.u = ur_enter(a, n, b, t, entry, lds, &p.s);
    uint32_t summed;
    p.o0 = block_excl_add(bzd_ur_size(p.u.w, p.u.cnt, p.u.prev, p.s, &p.s_end), lds, &summed);
    p.lim = min(tile_total, summed);
    return p;
}

// n bytes of LDS to global memory by the `nth` threads of which this is thread `tid`: aligned words, the ragged edges byte by byte
__device__ __forceinline__ void ur_copy_out(uint8_t *g, const uint8_t *s, uint32_t n, uint32_t tid, uint32_t nth)
{
    const uint32_t head = min(n, (uint32_t)((0 - (uintptr_t)g) & 3u));
    const uint32_t words = (n - head) / 4, tail0 = head + words * 4;
    if (tid < head) g[tid] = s[tid];
    for (uint32_t i = tid; i < words; i += nth) {
        const uint8_t *sp = s + head + 4 * i;
        *reinterpret_cast<uint32_t *>(g + head + 4 * i) = (uint32_t)sp[0] | (uint32_t)sp[1] << 8 | (uint32_t)sp[2] << 16 | (uint32_t)sp[3] << 24;
    }
    if (tail0 + tid < n) g[tail0 + tid] = s[tail0 + tid];
}

__global__ void __launch_bounds__(UR_THREADS) unrle_maps(UrArgs a)
{
    __shared__ uint32_t lds[4];
    const uint32_t b = a.slots[blockIdx.y], t = blockIdx.x, n = a.n[b];
    const UrBytes u = ur_load(a.x + (size_t)b * a.S, n, t * UR_TILE + threadIdx.x * UR_ITEMS);
    uint32_t total;
    (void)ur_scan(bzd_ur_map(u.w, u.cnt, u.prev), lds, &total);
    if (threadIdx.x == 0) a.tmap[(size_t)b * a.T + t] = total;
}

template <bool EXPAND>
__global__ void __launch_bounds__(UR_THREADS) unrle_walk(UrArgs a)
{
    __shared__ uint32_t lds[8];
    __shared__ uint8_t stage[EXPAND ? UR_STAGE : 4];
    const uint32_t b = a.slots[blockIdx.y], t = blockIdx.x, n = a.n[b];
    const size_t ti = (size_t)b * a.T + t;
    uint32_t entry, tile_total = 0xFFFFFFFFu;
    if (EXPAND) {
        entry = a.tstate[ti];
        tile_total = a.tout[ti];
        if (tile_total == 0) return;
    } else { // the tiles before this one, a thread each (T <= UR_THREADS: dec_ws's static_assert)
        uint32_t total;
        const uint32_t m = threadIdx.x < t ? a.tmap[(size_t)b * a.T + threadIdx.x] : BZD_RL_ID;
        (void)ur_scan(m, lds, &total);
        entry = bzd_rl_apply(total, 0);
        if (threadIdx.x == 0) a.tstate[ti] = entry;
    }
    const UrPlace p = ur_place(a, n, b, t, entry, tile_total, lds);
    const UrBytes &u = p.u;
    if (!EXPAND) {
        if (threadIdx.x == 0) a.tout[ti] = p.lim;
        if (u.cnt && t * UR_TILE + threadIdx.x * UR_ITEMS + u.cnt == n) a.endstate[b] = p.s_end;
        return;
    }
    const bool staged = tile_total <= UR_STAGE;
    uint8_t *g = a.out + a.obase[blockIdx.y] + a.toff[ti];
    // A loop of its own, a byte and a test at a time, where unrle_walk_win and unrle_walk_pieces go through bzd_ur_emit.  On text,
    // where nearly every byte stands for itself, bzd_ur_emit's loop per byte of input made this kernel 8 % slower and the stage
    // 3 %; on long runs bzd_ur_emit is five times faster here (profiles/r27_unrle_front_ab.txt has both).
    uint32_t o = p.o0, s = p.s, prev = u.prev;
#pragma unroll
    for (int k = 0; k < (int)UR_ITEMS; k++) {
        if ((uint32_t)k < u.cnt) {
            const uint32_t c = bzd_ur_at(u.w, k);
            if (s == 4) {
                for (uint32_t q = 0; q < c; q++, o++)
                    if (o < p.lim) {
                        if (staged)
                            stage[o] = (uint8_t)prev;
                        else
                            g[o] = (uint8_t)prev;
                    }
            } else {
                if (o < p.lim) {
                    if (staged)
                        stage[o] = (uint8_t)c;
                    else
                        g[o] = (uint8_t)c;
                }
                o++;
            }
            s = bzd_rl_step(s, c == prev);
            prev = c;
        }
    }
    if (!staged) return;
    __syncthreads();
    ur_copy_out(g, stage, p.lim, threadIdx.x, UR_THREADS);
}

// ---- random access: the expansion clipped to a window, and its CRC without the expansion -------------------------------
struct UwArgs {
    const uint32_t *wlo, *whi; // [K] the window of the block, in bytes of its own output
    const int64_t *wbase;      // [K] out + wbase = where the block's first byte would lie (before `out` when the window cuts its head)
    const uint32_t *bsize;     // [K] decoded bytes of the block
    uint32_t *acc, *crc;       // [K] CRC accumulator (zeroed by the host), finished CRC
    const CrcTables *ct;
};

// unrle_walk<true> for a block of which only [wlo, whi) is wanted.  Not one byte outside the window is stored: the staged tile
// is copied out from the window's first byte to its last, the byte stores of a tile too large to stage are clipped run by run.
__global__ void __launch_bounds__(UR_THREADS) unrle_walk_win(UrArgs a, UwArgs wa)
{
    __shared__ uint32_t lds[8];
    __shared__ uint8_t stage[UR_STAGE];
    const uint32_t b = a.slots[blockIdx.y], t = blockIdx.x, n = a.n[b];
    const size_t ti = (size_t)b * a.T + t;
    const uint32_t tile_total = a.tout[ti];
    if (tile_total == 0) return;
    const uint32_t toff = a.toff[ti], lo = wa.wlo[blockIdx.y], hi = wa.whi[blockIdx.y];
    uint32_t ca, cb;
    bzd_clip(toff, tile_total, lo, hi, &ca, &cb);
    if (ca == cb) return; // the tile lies outside the window
    const uint32_t tlo = ca - toff, thi = cb - toff; // the window inside the tile
    const UrPlace p = ur_place(a, n, b, t, a.tstate[ti], tile_total, lds);
    const UrBytes &u = p.u;
    const uint32_t whi_t = min(thi, p.lim);
    uint8_t *g = reinterpret_cast<uint8_t *>((uintptr_t)a.out + (uintptr_t)(wa.wbase[blockIdx.y] + (int64_t)toff));
    if (tile_total > UR_STAGE) {
        bzd_ur_emit(u.w, u.cnt, u.prev, p.s, p.o0, tlo, whi_t, [&](uint32_t q, uint8_t v) { g[q] = v; });
        return;
    }
    bzd_ur_emit(u.w, u.cnt, u.prev, p.s, p.o0, tlo, whi_t, [&](uint32_t q, uint8_t v) { stage[q] = v; });
    __syncthreads();
    if (whi_t > tlo) ur_copy_out(g + tlo, stage + tlo, whi_t - tlo, threadIdx.x, UR_THREADS);
}

// ---- many ranges: one expansion of a tile, many destinations --------------------------------------------------------------
struct UpArgs {
    const uint32_t *tile_first; // [K * Tp + 1] bzp_pieces' table: the references of tile t of block k
    const PieceRef *refs;       // each cut to its tile, in the block's own output coordinates
    uint32_t Tp, nrefs;
    uint64_t out_total;         // bytes of `out`: no store at or behind it
};

// unrle_walk_win for a block of which several pieces are wanted, each somewhere else: the tile is loaded, scanned and expanded
// once, then stage[piece] goes to every piece that meets the tile -- a wavefront a piece where there are many, the workgroup
// where there are few.  A tile too large to stage is emitted piece by piece, clipped run by run.  No reference is trusted: every
// position is clipped to the reference, to the tile's total and to this walk's own sum, every destination to out_total.
__global__ void __launch_bounds__(UR_THREADS) unrle_walk_pieces(UrArgs a, UpArgs pa)
{
    __shared__ uint32_t lds[8];
    __shared__ uint8_t stage[UR_STAGE];
    const uint32_t b = a.slots[blockIdx.y], t = blockIdx.x, n = a.n[b];
    const size_t ti = (size_t)b * a.T + t;
    const uint32_t tile_total = a.tout[ti];
    if (tile_total == 0 || t >= pa.Tp) return;
    const size_t cell = (size_t)blockIdx.y * pa.Tp + t;
    const uint32_t f1 = min(pa.tile_first[cell + 1], pa.nrefs), f0 = min(pa.tile_first[cell], f1);
    if (f0 == f1) return; // no piece meets the tile
    const uint32_t toff = a.toff[ti];
    const UrPlace p = ur_place(a, n, b, t, a.tstate[ti], tile_total, lds);
    const UrBytes &u = p.u;
    const uint32_t s = p.s, o0 = p.o0, lim = p.lim;
    const bool staged = tile_total <= UR_STAGE;
    if (staged) {
        bzd_ur_emit(u.w, u.cnt, u.prev, s, o0, 0u, lim, [&](uint32_t q, uint8_t v) { stage[q] = v; });
        __syncthreads();
    }
    // (bzd_piece_cut: the piece inside the tile, [ca, cb) of the tile's own bytes, and where its first byte goes)
    auto cut = [&](const PieceRef &r, uint32_t *ca, uint32_t *cb, uint8_t **g) {
        uint64_t dst;
        if (!bzd_piece_cut(toff, lim, r.lo, r.hi, r.base, pa.out_total, ca, cb, &dst)) return false;
        *g = a.out + dst;
        return true;
    };
    uint32_t ca, cb;
    uint8_t *g;
    if (!staged) {
        for (uint32_t f = f0; f < f1; f++)
            if (cut(pa.refs[f], &ca, &cb, &g)) bzd_ur_emit(u.w, u.cnt, u.prev, s, o0, ca, cb, [&](uint32_t q, uint8_t v) { g[q - ca] = v; });
    } else if (f1 - f0 < UR_THREADS / 64) {
        for (uint32_t f = f0; f < f1; f++)
            if (cut(pa.refs[f], &ca, &cb, &g)) ur_copy_out(g, stage + ca, cb - ca, threadIdx.x, UR_THREADS);
    } else {
        for (uint32_t f = f0 + (threadIdx.x >> 6); f < f1; f += UR_THREADS / 64)
            if (cut(pa.refs[f], &ca, &cb, &g)) ur_copy_out(g, stage + ca, cb - ca, threadIdx.x & 63u, 64);
    }
}

// The CRC of a block's expansion from the bytes behind its inverse BWT.  The CRC is linear: a thread folds what its 16 bytes
// stand for (literals and runs, entered in the state the scan hands it) into a register of its own, and that register times
// x^(8 * bytes behind the thread's piece in the block) is the piece's share of the block's CRC.  The power splits in two: the
// bytes behind the piece inside the tile (below 2^20: a product over the set bits, a thread each) and the bytes behind the tile
// (one gf_pow_x a tile, wave 0).  The shares are XORed: over the workgroup, then into the block's accumulator.
__global__ void __launch_bounds__(UR_THREADS) unrle_crc(UrArgs a, UwArgs wa)
{
    __shared__ uint32_t lds[8];
    __shared__ uint32_t tab[256];
    __shared__ uint32_t wred[UR_THREADS / 64];
    const uint32_t b = a.slots[blockIdx.y], t = blockIdx.x, n = a.n[b];
    const size_t ti = (size_t)b * a.T + t;
    const uint32_t tile_total = a.tout[ti];
    if (tile_total == 0) return;
    {
        uint32_t c = threadIdx.x << 24;
#pragma unroll
        for (int k = 0; k < 8; k++) c = (c << 1) ^ ((c >> 31) ? CRC_POLY : 0u);
        tab[threadIdx.x] = c;
    }
    uint32_t s, outn, summed;
    const UrBytes u = ur_enter(a, n, b, t, a.tstate[ti], lds, &s); // (its barriers also publish the table)
    uint32_t crc = bzd_ur_fold(tab, u.w, u.cnt, u.prev, s, &outn);
    const uint32_t o0 = block_excl_add(outn, lds, &summed);
    if (outn) crc = gf_mul(crc, gf_pow_x_serial(wa.ct->pow2 + 3, summed - o0 - outn, 20)); // x^(8 m), m < 4096 * 255 < 2^20
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) crc ^= __shfl_xor(crc, d, 64);
    if ((threadIdx.x & 63u) == 0) wred[threadIdx.x >> 6] = crc;
    __syncthreads();
    if (threadIdx.x < 64) {
        uint32_t c = 0;
        for (uint32_t k = 0; k < UR_THREADS / 64; k++) c ^= wred[k];
        const uint32_t bs = wa.bsize[blockIdx.y], behind = a.toff[ti] + summed; // (the host has checked that the tiles sum to bsize)
        const uint32_t pw = gf_pow_x(*wa.ct, 8ull * (bs > behind ? bs - behind : 0u), threadIdx.x);
        if (threadIdx.x == 0) atomicXor(&wa.acc[blockIdx.y], gf_mul(c, pw));
    }
}

// init and final XOR of CRC-32/BZIP2, as crc_finish (rle1.hip) folds them in
__global__ void __launch_bounds__(64) unrle_crc_finish(UwArgs wa)
{
    const uint32_t pw = gf_pow_x(*wa.ct, 8ull * wa.bsize[blockIdx.x], threadIdx.x);
    if (threadIdx.x == 0) wa.crc[blockIdx.x] = wa.acc[blockIdx.x] ^ gf_mul(0xFFFFFFFFu, pw) ^ 0xFFFFFFFFu;
}

// ---- records: the delimiters of a block's expansion, counted and located from the bytes behind its inverse BWT ----------------
struct UcArgs {
    uint32_t delim;
    uint32_t *tcount; // [B][T] delimiters the tile expands to
    uint32_t *last;   // [B] the block's last output byte is the delimiter
};

// unrle_crc's grid and entry states, folding a count instead of a CRC: what a thread's 16 bytes stand for (bzd_ur_count), summed
// over the workgroup and stored plainly, a word a tile -- the host sums the tiles, and unrle_select wants them one by one.
__global__ void __launch_bounds__(UR_THREADS) unrle_count(UrArgs a, UcArgs ca)
{
    __shared__ uint32_t lds[8];
    __shared__ uint32_t wred[UR_THREADS / 64];
    const uint32_t b = a.slots[blockIdx.y], t = blockIdx.x, n = a.n[b];
    const size_t ti = (size_t)b * a.T + t;
    uint32_t s0, outn, last = 256;
    const UrBytes u = ur_enter(a, n, b, t, a.tstate[ti], lds, &s0);
    uint32_t d = bzd_ur_count(u.w, u.cnt, u.prev, s0, ca.delim, &outn, &last);
    if (u.cnt && t * UR_TILE + threadIdx.x * UR_ITEMS + u.cnt == n) ca.last[b] = last == ca.delim; // (one thread of one tile holds the block's last byte)
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) d += __shfl_xor(d, s, 64);
    if ((threadIdx.x & 63u) == 0) wred[threadIdx.x >> 6] = d;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0;
        for (uint32_t k = 0; k < UR_THREADS / 64; k++) c += wred[k];
        ca.tcount[ti] = c; // (a tile behind the block's last counts nothing: every word of the grid is written)
    }
}

struct UsArgs {
    const BzqQuery *q;
    uint32_t *pos; // [queries] the delimiter's position in its block's output, BZQ_NONE where no thread holds it
    uint32_t nslots, delim;
};

// One workgroup a query: the k-th delimiter of one tile.  The same load and scan, an exclusive sum of the threads' counts, and the
// one thread whose share holds the k-th walks its 16 bytes again (bzd_ur_select).  Whatever the query holds, every read is
// bounded by n[b] inside the slot's stride and the only store is the query's own word.
__global__ void __launch_bounds__(UR_THREADS) unrle_select(UrArgs a, UsArgs sa)
{
    __shared__ uint32_t lds[8];
    __shared__ uint32_t found;
    const BzqQuery q = sa.q[blockIdx.x];
    if (threadIdx.x == 0) found = BZQ_NONE;
    if (q.slot >= sa.nslots || q.tile >= a.T) { // (the same for every thread)
        if (threadIdx.x == 0) sa.pos[blockIdx.x] = BZQ_NONE;
        return;
    }
    const uint32_t b = q.slot, n = min(a.n[b], a.S);
    const size_t ti = (size_t)b * a.T + q.tile;
    uint32_t s, outn, last = 256, dsum, osum;
    const UrBytes u = ur_enter(a, n, b, q.tile, a.tstate[ti], lds, &s); // (its barriers also publish `found`)
    const uint32_t d = bzd_ur_count(u.w, u.cnt, u.prev, s, sa.delim, &outn, &last);
    const uint32_t d0 = block_excl_add(d, lds, &dsum);
    const uint32_t o0 = block_excl_add(outn, lds, &osum);
    if (q.k > d0 && q.k - d0 <= d) found = a.toff[ti] + o0 + bzd_ur_select(u.w, u.cnt, u.prev, s, sa.delim, q.k - d0);
    __syncthreads();
    if (threadIdx.x == 0) sa.pos[blockIdx.x] = found;
}

// The same table from decoded bytes (bzh_count_records_device): the delimiters of raw[offs[e], offs[e] + lens[e]), a word a tile
// of CB_TILE bytes, summed on the host.  No state machine: aligned 16-byte loads, the ragged edges byte by byte, one reduction a
// workgroup.  The host has checked that every entry lies inside the buffer.
constexpr uint32_t CB_THREADS = 256, CB_TILE = 16384;

__device__ __forceinline__ uint32_t cb_eq4(uint32_t w, uint32_t pat) // bytes of w equal to the byte pat repeats
{
    const uint32_t x = w ^ pat;
    return (uint32_t)__popc(~((((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) | 0x7F7F7F7Fu));
}

// (the grid is the tiles of all entries end to end, tfirst[e] = the first tile of entry e, tfirst[count] = their number: the work
// is the bytes' whatever the entries' sizes are)
__global__ void __launch_bounds__(CB_THREADS) count_bytes_blocks(const uint8_t *raw, const uint64_t *offs, const uint32_t *lens,
                                                                  const uint32_t *tfirst, uint32_t count, uint32_t delim, uint32_t *tcount)
{
    __shared__ uint32_t wred[CB_THREADS / 64];
    uint32_t e = 0, hi = count - 1; // the last entry whose first tile is this one or lies in front of it
    while (e < hi) {
        const uint32_t mid = e + (hi - e + 1) / 2;
        if (tfirst[mid] <= blockIdx.x)
            e = mid;
        else
            hi = mid - 1;
    }
    const uint32_t t = blockIdx.x - tfirst[e], len = lens[e], lo = t * CB_TILE;
    uint32_t c = 0;
    if (t < (len + CB_TILE - 1) / CB_TILE) {
        const uint8_t *p = raw + offs[e] + lo;
        const uint32_t m = min(CB_TILE, len - lo), head = min(m, (uint32_t)((0 - (uintptr_t)p) & 15u));
        const uint32_t nv = (m - head) / 16, tail0 = head + nv * 16, pat = delim * 0x01010101u;
        if (threadIdx.x < head) c += p[threadIdx.x] == delim;
        for (uint32_t i = threadIdx.x; i < nv; i += CB_THREADS) {
            const uint4 v = *reinterpret_cast<const uint4 *>(p + head + 16 * i);
            c += cb_eq4(v.x, pat) + cb_eq4(v.y, pat) + cb_eq4(v.z, pat) + cb_eq4(v.w, pat);
        }
        if (tail0 + threadIdx.x < m) c += p[tail0 + threadIdx.x] == delim;
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) c += __shfl_xor(c, s, 64);
    if ((threadIdx.x & 63u) == 0) wred[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) tcount[blockIdx.x] = wred[0] + wred[1] + wred[2] + wred[3];
}

// bad[k] = the 48 bits at candidate k are not the block magic (the scan vouches for that in a full decode, an index entry does not)
__global__ void __launch_bounds__(64) range_magic_kernel(const uint8_t *in, uint64_t n, const uint64_t *cand, uint32_t B, uint32_t *bad)
{
    const uint32_t k = blockIdx.x * 64 + threadIdx.x;
    if (k >= B) return;
    const uint64_t pos = cand[k] >> 1, byte = pos >> 3;
    uint64_t v = 0;
    for (uint32_t j = 0; j < 7; j++) v = v << 8 | (byte + j < n ? (uint64_t)in[byte + j] : 0ull);
    bad[k] = ((v >> (8 - (pos & 7u))) & 0xFFFFFFFFFFFFull) != BZD_BLOCK_MAGIC || pos + 48 > n * 8;
}

// ---- host side ---------------------------------------------------------------------------------------------------
// unrle_walk sums the tiles in front of its own a thread each: no context's stride holds more tiles than the kernel has threads.
static_assert(batch_stride(100000u * 9u - 1u) / UR_TILE <= UR_THREADS, "a level-9 block's tiles exceed the walk kernel's threads");

static int dec_ws(bzh_ctx *ctx, DecWs &w)
{
    const uint32_t B = ctx->max_batch, T = ctx->S / UR_TILE;
    BZH_TRY(ctx->dec_ws.reserve(ctx, dec_layout(w, nullptr, B, T), "the decode tables"));
    dec_layout(w, ctx->dec_ws, B, T);
    return BZH_OK;
}

// The blocks a batch may hold: the context's, and no more than the arena was sized for.
static uint32_t batch_max(const bzh_ctx *ctx) { return (uint32_t)std::min<size_t>(ctx->max_batch, ctx->arena_blocks); }

// The recorder's workspace is bounded by shrinking the batch, whatever the interval: a slot holds every point a block can have,
// (BZD_MAX_SEL - 1) / interval of 288 bytes -- 9.4 MB at interval 1 -- and a batch has as many slots as fit in this many bytes.
constexpr size_t SYNC_REC_BYTES = 64u << 20;

// Every magic in d_in[0..n): (bit position << 1 | kind), ascending.
int decode_scan_run(bzh_ctx *ctx, const uint8_t *d_in, size_t n, std::vector<uint64_t> &cands)
{
    hipStream_t st = ctx->stream;
    DecWs w;
    BZH_TRY(dec_ws(ctx, w));
    cands.clear();
    if (n < 6) return BZH_OK;
    const uint64_t wgs = (n + (uint64_t)SCAN_THREADS * SCAN_BYTES - 1) / ((uint64_t)SCAN_THREADS * SCAN_BYTES);
    if (wgs > 0x7FFFFFFFull) {
        bzh_set_error(ctx, "decode: an input of %zu bytes is beyond one scan launch", n);
        return BZH_E_ARG;
    }
    size_t list_cap = std::max<size_t>(65536, ctx->dec_list.cap / 8); // hits the list holds
    for (int attempt = 0; attempt < 2; attempt++) {
        BZH_TRY(ctx->dec_list.reserve(ctx, list_cap * 8, "the scan's hit list"));
        HIP_TRY(ctx, hipMemsetAsync(w.scancnt, 0, 4, st));
        decode_scan_kernel<<<dim3((uint32_t)wgs), SCAN_THREADS, 0, st>>>(d_in, n, ctx->dec_list.as<uint64_t>(), (uint32_t)list_cap, w.scancnt);
        HIP_TRY(ctx, hipGetLastError());
        uint32_t cnt = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&cnt, w.scancnt, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, bzh_stream_wait(st));
        if (cnt <= list_cap) {
            cands.resize(cnt);
            if (cnt) HIP_TRY(ctx, hipMemcpy(cands.data(), ctx->dec_list, (size_t)cnt * 8, hipMemcpyDeviceToHost));
            std::sort(cands.begin(), cands.end());
            return BZH_OK;
        }
        list_cap = (size_t)cnt + 1024; // more hits than the list holds: once more with one that does
    }
    bzh_set_error(ctx, "decode: the scan's hit list overflowed twice (internal error)");
    return BZH_E_STATE;
}

static const char *kind_name(uint32_t k)
{
    switch (k) {
    case BZD_K_MAGIC: return "bad magic";
    case BZD_K_TRUNC: return "truncated stream";
    case BZD_K_FORMAT: return "field outside the format";
    case BZD_K_BLOCK_CRC: return "block CRC mismatch";
    case BZD_K_STREAM_CRC: return "stream CRC mismatch";
    case BZD_K_RANDOMISED: return "randomised block (not supported)";
    default: return "error";
    }
}

namespace {
struct StageSpan {
    int stage;
    hipEvent_t a, b;
};
struct ChainItem { // what the chain walk met in a batch, in order
    bool footer;
    uint32_t slot;   // block: its batch slot
    uint32_t crc;    // stored CRC
    size_t stream, block;
    uint64_t bitpos;
    uint64_t end_bit; // first bit behind it
    uint32_t level;   // of its stream
};
struct StageClock { // HIP events around the stages of a decode call, summed into bzh_decode_stats when profiling is on
    bzh_ctx *ctx;
    std::vector<StageSpan> spans;
    hipEvent_t mark()
    {
        if (!ctx->profiling) return nullptr;
        hipEvent_t e = bzh_event(ctx);
        hipEventRecord(e, ctx->stream);
        return e;
    }
    void span(int stage, hipEvent_t a)
    {
        if (a) spans.push_back({stage, a, mark()});
    }
    void collect()
    {
        bzh_decode_stats &ds = ctx->dstats;
        double *dst[6] = {&ds.ms_scan, &ds.ms_entropy, &ds.ms_unbwt, &ds.ms_unrle, &ds.ms_crc, &ctx->mstats.ms_unbwt_small};
        for (auto &s : spans) {
            float t = 0;
            if (hipEventElapsedTime(&t, s.a, s.b) == hipSuccess) *dst[s.stage] += t;
        }
        spans.clear();
    }
};
} // namespace

// ---- the back of the decoder: inverse BWT, inverse RLE1, block CRCs -- one place, in two steps, because the host has to know
// every block's size before anything can be placed.  decode_chain_run and decode_range_run both go through it.
struct BackBlock {
    uint32_t slot, nblock; // in: its batch slot, the bytes of its last column
    uint64_t size;         // back_sizes: its decoded bytes
    bool bad_end;          // back_sizes: it ends in state 4, four equal bytes without a count (libbz2 refuses the block)
    int64_t base;          // back_emit, in: out + base = where its first byte lies (before `out` when the window cuts its head)
    uint32_t lo, hi;       // back_emit, in: the window wanted, in bytes of its own output
    uint32_t crc;          // back_emit: of all its decoded bytes, whatever the window
    bool whole() const { return lo == 0 && hi == size; }
};
struct Back { // a batch between its two steps; the vectors are scratch kept from batch to batch
    UrArgs a;
    uint32_t Tn;
    hipEvent_t t_unrle; // the unrle stage's span opens in back_sizes; back_emit closes it, or the caller that stops at the sizes
    std::vector<uint32_t> hslots, hout, hend, hoff, fq, eq, fslots, eslots, elo, ehi, esize, ecrc, hsmall;
    std::vector<uint64_t> fbase;
    std::vector<int64_t> ebase;
    std::vector<BlockDesc> fdesc;
};

// Step one.  The inverse BWT of batch slots [0, Bu), blocks of up to nmax_all bytes -- a chain's batch also holds candidates
// off the chain that decoded cleanly, and the transform runs over slots, not over a list --, then the state maps and sizes of
// the listed blocks.  One copy back, one wait; bk.hoff is the host image of toff.  Reports nothing: the callers word the errors.
// split (bzh_decode_many only): the listed blocks of at most split->small_max bytes go through the LDS transform, which takes a
// list and so leaves the candidates off the chain alone; unbwt_run then runs over slots [0, split->Bl) only -- up to the last
// listed block above the bound, sized by split->nmax_l -- and first: where both write a small block's slot they write the same.
struct BackCount { // the delimiters of the listed blocks beside their sizes or CRCs (unrle_count): a record table, a read by records
    uint32_t delim;
    uint32_t *d_tcount, *d_last; // [B][T], [B] device (ctx->records_ws)
    std::vector<uint32_t> tcount, last; // their host images, by batch slot, behind the step's wait
};
// queued behind the kernels that leave the entry states; `a` names the blocks' slots, Bu = slots the images cover
static int back_count_queue(bzh_ctx *ctx, const UrArgs &a, uint32_t Tn, uint32_t K, uint32_t Bu, BackCount &bc)
{
    hipStream_t st = ctx->stream;
    unrle_count<<<dim3(Tn, K), UR_THREADS, 0, st>>>(a, UcArgs{bc.delim, bc.d_tcount, bc.d_last});
    HIP_TRY(ctx, hipGetLastError());
    bc.tcount.resize((size_t)Bu * a.T);
    bc.last.resize(Bu);
    HIP_TRY(ctx, hipMemcpyAsync(bc.tcount.data(), bc.d_tcount, bc.tcount.size() * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(bc.last.data(), bc.d_last, (size_t)Bu * 4, hipMemcpyDeviceToHost, st));
    return BZH_OK;
}
// the two tables, for batches of the context's size (the stream is idle between batches)
// and, for a read, its queries and their answers: nq of each at most in the whole call, so nothing moves between its batches
static int back_count_ws(bzh_ctx *ctx, BackCount &bc, size_t nq = 0, BzqQuery **d_q = nullptr, uint32_t **d_pos = nullptr)
{
    const size_t B = ctx->max_batch, T = ctx->S / UR_TILE;
    BzqQuery *q = nullptr;
    uint32_t *pos = nullptr;
    BZH_TRY(reserve_cut(ctx, ctx->records_ws, "the record tables", grow_mib, [&](Carver &c) {
        c.put(q, nq), c.put(bc.d_tcount, B * T), c.put(bc.d_last, B), c.put(pos, nq);
    }));
    if (d_q) *d_q = q;
    if (d_pos) *d_pos = pos;
    return BZH_OK;
}
struct BackSplit {
    uint32_t small_max;
    uint32_t Bl, nmax_l; // Bl 0: no listed block above the bound
    uint32_t nsmall;     // out: blocks the LDS transform took
};
static int back_sizes(bzh_ctx *ctx, const DecWs &w, StageClock &clock, Back &bk, uint32_t Bu, uint32_t nmax_all, std::vector<BackBlock> &blocks,
                      BackSplit *split = nullptr, BackCount *count = nullptr)
{
    hipStream_t st = ctx->stream;
    const Batch &bt = ctx->bt;
    const uint32_t K = (uint32_t)blocks.size();
    uint32_t nmax = 1;
    bk.hslots.clear();
    for (const BackBlock &b : blocks) {
        bk.hslots.push_back(b.slot);
        nmax = std::max(nmax, b.nblock);
    }
    hipEvent_t t2 = clock.mark();
    if (!split) {
        BZH_TRY(unbwt_run(ctx, Bu, nmax_all));
    } else {
        if (split->Bl) BZH_TRY(unbwt_run(ctx, split->Bl, split->nmax_l));
        bk.hsmall.clear();
        for (const BackBlock &b : blocks)
            if (b.nblock <= split->small_max) bk.hsmall.push_back(b.slot);
        split->nsmall = (uint32_t)bk.hsmall.size();
        if (split->nsmall) {
            HIP_TRY(ctx, hipMemcpyAsync(w.small, bk.hsmall.data(), (size_t)split->nsmall * 4, hipMemcpyHostToDevice, st));
            hipEvent_t t5 = clock.mark();
            BZH_TRY(unbwt_small_run(ctx, w.small, split->nsmall));
            clock.span(5, t5);
        }
    }
    clock.span(2, t2);
    bk.t_unrle = clock.mark();
    bk.a = UrArgs{bt.unbwt_out, bt.n, w.slots, bt.S, w.T, w.tmap, w.tout, w.tstate, w.endstate, w.toff, w.obase, nullptr};
    bk.Tn = (nmax + UR_TILE - 1) / UR_TILE;
    HIP_TRY(ctx, hipMemcpyAsync(w.slots, bk.hslots.data(), (size_t)K * 4, hipMemcpyHostToDevice, st));
    unrle_maps<<<dim3(bk.Tn, K), UR_THREADS, 0, st>>>(bk.a);
    unrle_walk<false><<<dim3(bk.Tn, K), UR_THREADS, 0, st>>>(bk.a);
    HIP_TRY(ctx, hipGetLastError());
    bk.hout.resize((size_t)Bu * w.T);
    bk.hend.resize(Bu);
    HIP_TRY(ctx, hipMemcpyAsync(bk.hout.data(), w.tout, bk.hout.size() * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(bk.hend.data(), w.endstate, (size_t)Bu * 4, hipMemcpyDeviceToHost, st));
    if (count) BZH_TRY(back_count_queue(ctx, bk.a, bk.Tn, K, Bu, *count)); // (a read by records: before this step's wait, not behind one of its own)
    HIP_TRY(ctx, bzh_stream_wait(st));
    bk.hoff.assign((size_t)Bu * w.T, 0);
    for (BackBlock &b : blocks) {
        b.size = bzp_tile_sums(bk.hout.data() + (size_t)b.slot * w.T, bk.hoff.data() + (size_t)b.slot * w.T, b.nblock, UR_TILE);
        b.bad_end = bk.hend[b.slot] == 4;
    }
    return BZH_OK;
}

// Step two, over the list back_sizes filled (every block, same order), each with its base and window.  A window that is the
// whole block: expanded where it belongs and checked there (unrle_walk<true>, crc_blocks_device).  A part of it: clipped
// (unrle_walk_win), and its CRC folded from the bytes behind the inverse BWT with nothing more written (unrle_crc).  Empty: the
// CRC alone -- the index build.  Only the kernels some block needs are launched.  crcs false: no CRC is taken.  One wait.
// relist: `blocks` is not the list back_sizes was given but some of its blocks (bzh_recover's second emit, of the blocks the first
// one's CRCs kept): the whole blocks' slots go up again.
// pieces (bzh_decode_ranges only): blocks of the list with an empty window here, emitted piece by piece beside the others.
// count (bzh_decode_index_records only): the delimiters of the blocks with nothing to write, where their CRCs are folded.
struct BackPieces {
    const uint32_t *slots; // [K] device: their batch slots
    uint32_t K;
    UpArgs args;
};
static int back_emit(bzh_ctx *ctx, const DecWs &w, StageClock &clock, Back &bk, uint8_t *d_out, bool crcs, std::vector<BackBlock> &blocks,
                     bool relist = false, const BackPieces *pieces = nullptr, BackCount *count = nullptr)
{
    hipStream_t st = ctx->stream;
    auto up = [&](void *dst, const void *src, size_t bytes) { return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st); };
    bk.fq.clear(), bk.fslots.clear(), bk.fbase.clear(), bk.fdesc.clear();
    bk.eq.clear(), bk.eslots.clear(), bk.elo.clear(), bk.ehi.clear(), bk.esize.clear(), bk.ebase.clear();
    uint64_t maxsize = 0;
    uint32_t KW = 0; // whole blocks; cut blocks; behind them, where the clipped walk does not look, the blocks with nothing to write
    for (int pass = 0; pass < (crcs ? 3 : 2); pass++)
        for (uint32_t q = 0; q < blocks.size(); q++) {
            const BackBlock &b = blocks[q];
            if ((b.whole() ? 0 : b.lo < b.hi ? 1 : 2) != pass) continue;
            if (pass == 0) {
                bk.fq.push_back(q), bk.fslots.push_back(b.slot), bk.fbase.push_back((uint64_t)b.base);
                bk.fdesc.push_back(BlockDesc{(uint64_t)b.base, b.size, 0, 0});
                maxsize = std::max(maxsize, b.size);
            } else {
                bk.eq.push_back(q), bk.eslots.push_back(b.slot), bk.esize.push_back((uint32_t)b.size);
                bk.elo.push_back(b.lo), bk.ehi.push_back(b.hi), bk.ebase.push_back(b.base);
                KW += pass == 1;
            }
        }
    const uint32_t KF = (uint32_t)bk.fq.size(), KE = (uint32_t)bk.eq.size();
    UrArgs &a = bk.a, ae = bk.a;
    a.out = ae.out = d_out;
    ae.slots = w.wslots;
    UwArgs wa{w.wlo, w.whi, w.wbase, w.bsize, w.wacc, w.wcrc, nullptr};
    HIP_TRY(ctx, up(w.toff, bk.hoff.data(), bk.hoff.size() * 4));
    if (KF) {
        if (KF != blocks.size() || relist) HIP_TRY(ctx, up(w.slots, bk.fslots.data(), (size_t)KF * 4)); // (else it holds them since back_sizes)
        HIP_TRY(ctx, up(w.obase, bk.fbase.data(), (size_t)KF * 8));
        unrle_walk<true><<<dim3(bk.Tn, KF), UR_THREADS, 0, st>>>(a);
    }
    if (KE) HIP_TRY(ctx, up(w.wslots, bk.eslots.data(), (size_t)KE * 4));
    if (KW) {
        HIP_TRY(ctx, up(w.wlo, bk.elo.data(), (size_t)KW * 4));
        HIP_TRY(ctx, up(w.whi, bk.ehi.data(), (size_t)KW * 4));
        HIP_TRY(ctx, up(w.wbase, bk.ebase.data(), (size_t)KW * 8));
        unrle_walk_win<<<dim3(bk.Tn, KW), UR_THREADS, 0, st>>>(ae, wa);
    }
    if (pieces && pieces->K) {
        UrArgs ap = bk.a;
        ap.slots = pieces->slots;
        unrle_walk_pieces<<<dim3(bk.Tn, pieces->K), UR_THREADS, 0, st>>>(ap, pieces->args);
    }
    HIP_TRY(ctx, hipGetLastError());
    clock.span(3, bk.t_unrle);
    hipEvent_t t4 = clock.mark();
    if (crcs && KF) {
        HIP_TRY(ctx, up(w.desc, bk.fdesc.data(), (size_t)KF * sizeof(BlockDesc)));
        BZH_TRY(crc_blocks_device(ctx, d_out, w.desc, w.crcacc, KF, maxsize));
        HIP_TRY(ctx, hipMemcpyAsync(bk.fdesc.data(), w.desc, (size_t)KF * sizeof(BlockDesc), hipMemcpyDeviceToHost, st));
    }
    bk.ecrc.resize(KE);
    if (crcs && KE) {
        BZH_TRY(crc_tables(ctx, &wa.ct));
        HIP_TRY(ctx, up(w.bsize, bk.esize.data(), (size_t)KE * 4));
        HIP_TRY(ctx, hipMemsetAsync(w.wacc, 0, (size_t)KE * 4, st));
        unrle_crc<<<dim3(bk.Tn, KE), UR_THREADS, 0, st>>>(ae, wa);
        unrle_crc_finish<<<dim3(KE), 64, 0, st>>>(wa);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(bk.ecrc.data(), w.wcrc, (size_t)KE * 4, hipMemcpyDeviceToHost, st));
    }
    if (count && KE > KW) { // (the blocks behind the cut ones in the list; their slots are what the images are indexed by)
        UrArgs ac = ae;
        ac.slots = w.wslots + KW;
        uint32_t Bu = 0;
        for (uint32_t e = KW; e < KE; e++) Bu = std::max(Bu, bk.eslots[e] + 1);
        BZH_TRY(back_count_queue(ctx, ac, bk.Tn, KE - KW, Bu, *count));
    }
    clock.span(4, t4);
    HIP_TRY(ctx, bzh_stream_wait(st));
    for (uint32_t f = 0; crcs && f < KF; f++) blocks[bk.fq[f]].crc = bk.fdesc[f].crc;
    for (uint32_t e = 0; crcs && e < KE; e++) blocks[bk.eq[e]].crc = bk.ecrc[e];
    return BZH_OK;
}

// The chain walk and the back of the decoder.  cands: decode_scan_run's list.  The arena holds min(cands, max_batch) blocks.
// index: the call builds a block index (bzh_decode_index*) -- cap is 0, nothing is expanded, every block's CRC comes from
// unrle_crc and is checked like a full decode's, and the entries are appended in chain order.
// sink: the call feeds a consumer of windows (bzh_search*, bzh_grep*: WindowSink, common.h) -- cap does not bound it, every batch is
// a window: its blocks are expanded at sink->front of the sink's staging buffer instead of at total_out in d_out, and behind the
// batch's CRC checks the sink is given the window.  The sink takes the whole output: begin(0, ~0, 0, 0), here and only here.
int decode_chain_run(bzh_ctx *ctx, const uint8_t *d_in, size_t n, uint8_t *d_out, size_t cap, size_t *out_len, size_t *consumed,
                     const std::vector<uint64_t> &cands, std::vector<bzh_index_entry> *index, SyncBuild *sync, RecBuild *rec, WindowSink *sink)
{
    if (sink) sink->begin(0, ~0ull, 0, 0);
    hipStream_t st = ctx->stream;
    Batch &bt = ctx->bt;
    bzh_decode_stats &ds = ctx->dstats;
    DecWs w;
    BZH_TRY(dec_ws(ctx, w));
    StageClock clock{ctx, {}};
    auto mark = [&]() { return clock.mark(); };
    auto span = [&](int stage, hipEvent_t a) { clock.span(stage, a); };
    size_t stream = 0, block = 0;
    auto data_error = [&](uint32_t kind, uint64_t bitpos, const char *what = nullptr) {
        bzh_set_error(ctx, "decode: %s%s%s in stream %zu, block %zu, at bit %llu", kind_name(kind), what ? ": " : "", what ? what : "", stream,
                      block, (unsigned long long)bitpos);
        return BZH_E_DATA;
    };
    auto level_error = [&](uint32_t lv) {
        bzh_set_error(ctx, "decode: stream %zu is of level %u, the context of level %d", stream, lv, ctx->level);
        return BZH_E_ARG;
    };
    *out_len = 0;
    if (consumed) *consumed = 0;
    uint8_t hdr[4] = {0, 0, 0, 0};
    if (n) HIP_TRY(ctx, hipMemcpyAsync(hdr, d_in, std::min<size_t>(n, 4), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, bzh_stream_wait(st));
    if (n < 4) return data_error(n && memcmp(hdr, "BZh", std::min<size_t>(n, 3)) != 0 ? BZD_K_MAGIC : BZD_K_TRUNC, n * 8, "no stream header");
    if (hdr[0] != 'B' || hdr[1] != 'Z' || hdr[2] != 'h' || hdr[3] < '1' || hdr[3] > '9') return data_error(BZD_K_MAGIC, 0, "no \"BZh1\"..\"BZh9\"");
    uint32_t level = hdr[3] - '0';
    if ((int)level > ctx->level) return level_error(level);
    // sync points: a region per batch slot, and no more slots than the workspace's bound holds
    uint32_t sync_cap = 0, sync_slots = 0;
    uint32_t *d_ptcnt = nullptr;
    bzh_sync_point *d_pts = nullptr;
    std::vector<uint32_t> hptcnt;
    if (sync) {
        sync_cap = std::max<uint32_t>(1u, (BZD_MAX_SEL - 1) / sync->interval);
        const size_t slot_bytes = (size_t)sync_cap * sizeof(bzh_sync_point);
        sync_slots = (uint32_t)std::max<size_t>(1, std::min<size_t>(batch_max(ctx), SYNC_REC_BYTES / slot_bytes));
        BZH_TRY(reserve_cut(ctx, ctx->sync_ws, "the sync points", grow_mib, [&](Carver &c) { c.put(d_ptcnt, sync_slots); c.put(d_pts, (size_t)sync_slots * sync_cap); }));
    }
    BackCount bc{rec ? rec->delim : 0u, nullptr, nullptr, {}, {}};
    if (rec) {
        BZH_TRY(back_count_ws(ctx, bc));
        rec->cum.assign(1, 0);
        rec->last_is_delim = false;
    }
    const size_t nc = cands.size();
    const uint64_t nbits = (uint64_t)n * 8;
    uint64_t pos = 32, total_out = 0, batch_bytes = 0;
    uint32_t stream_crc = 0;
    size_t ci = 0;
    bool finished = false, over = false;
    std::vector<BzdResult> res;
    std::vector<ChainItem> items;
    std::vector<BackBlock> blocks; // the blocks the chain met in a batch, in order
    Back bk;
    while (!finished) {
        while (ci < nc && (cands[ci] >> 1) < pos) {
            ds.candidates_off_chain++;
            ci++;
        }
        if (ci == nc || (cands[ci] >> 1) != pos) return data_error(pos + 48 > nbits ? BZD_K_TRUNC : BZD_K_MAGIC, pos, "neither a block nor a footer");
        uint32_t B = (uint32_t)std::min<size_t>(batch_max(ctx), nc - ci);
        if (sync) B = std::min(B, sync_slots);
        hipEvent_t e0 = mark();
        HIP_TRY(ctx, hipMemcpyAsync(w.cand, cands.data() + ci, (size_t)B * 8, hipMemcpyHostToDevice, st));
        if (sync)
            decode_block_sync_kernel<<<dim3(B), 64, 0, st>>>(d_in, n, w.cand, bt, w.res, 100000u * (uint32_t)ctx->level, sync->interval, d_pts,
                                                             sync_cap, d_ptcnt);
        else
            decode_block_kernel<<<dim3(B), 64, 0, st>>>(d_in, n, w.cand, bt, w.res, 100000u * (uint32_t)ctx->level);
        HIP_TRY(ctx, hipGetLastError());
        span(1, e0);
        res.resize(B);
        HIP_TRY(ctx, hipMemcpyAsync(res.data(), w.res, (size_t)B * sizeof(BzdResult), hipMemcpyDeviceToHost, st));
        if (sync) {
            hptcnt.resize(B);
            HIP_TRY(ctx, hipMemcpyAsync(hptcnt.data(), d_ptcnt, (size_t)B * 4, hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(ctx, bzh_stream_wait(st));
        // the chain through this batch
        items.clear();
        blocks.clear();
        uint32_t k = 0;
        for (; k < B && !finished; k++) {
            const uint64_t cpos = cands[ci + k] >> 1;
            if (cpos < pos) {
                ds.candidates_off_chain++;
                continue;
            }
            if (cpos != pos) return data_error(pos + 48 > nbits ? BZD_K_TRUNC : BZD_K_MAGIC, pos, "neither a block nor a footer");
            const BzdResult &r = res[k];
            if (r.kind != BZD_OK) return data_error(r.kind, r.errpos);
            if (!(cands[ci + k] & 1ull)) {
                if (r.nblock > 100000u * level) return data_error(BZD_K_FORMAT, cpos, "more bytes than the stream's block size");
                items.push_back({false, k, r.crc, stream, block, cpos, r.end_bit, level});
                blocks.push_back(BackBlock{k, r.nblock, 0, false, 0, 0, 0, 0});
                block++;
                ds.blocks++;
                pos = r.end_bit;
                continue;
            }
            items.push_back({true, k, r.crc, stream, block, cpos, r.end_bit, level});
            ds.streams++;
            if (consumed) *consumed = (size_t)(r.end_bit / 8);
            if (r.follow & 0x100u) { // the next stream: its errors are errors
                stream++;
                block = 0;
                level = r.follow & 15u;
                if ((int)level > ctx->level) return level_error(level);
                pos = r.end_bit + 32;
            } else {
                finished = true; // the input ends here, or foreign bytes follow
            }
        }
        ci += k;
        // the back of the decoder for the blocks on the chain
        if (!blocks.empty()) {
            const uint32_t Bu = blocks.back().slot + 1;
            uint32_t nmax_all = 1; // (the inverse BWT runs over slots: the clean candidates off the chain among them set its size too)
            for (uint32_t s = 0; s < Bu; s++)
                if (!(cands[ci - k + s] & 1ull) && res[s].kind == BZD_OK) nmax_all = std::max(nmax_all, res[s].nblock);
            BZH_TRY(back_sizes(ctx, w, clock, bk, Bu, nmax_all, blocks));
            batch_bytes = 0;
            for (BackBlock &b : blocks) {
                if (b.bad_end) { // libbz2 refuses the block; the state machine says where
                    for (const ChainItem &it : items)
                        if (!it.footer && it.slot == b.slot) {
                            stream = it.stream;
                            block = it.block;
                            return data_error(BZD_K_FORMAT, it.bitpos, "the block ends in four equal bytes without a count");
                        }
                }
                b.base = sink ? (int64_t)(sink->front + batch_bytes) : (int64_t)total_out;
                batch_bytes += b.size;
                total_out += b.size;
            }
            if (!sink && total_out > cap) over = true; // (sizing goes on: the caller learns the total)
            uint8_t *d_to = d_out;
            if (sink) BZH_TRY(sink->room(ctx, batch_bytes, &d_to)); // (the sizes are known: the staging grows to the batch)
            if (index || !over) { // an index: the CRCs of the expansions, with nothing expanded
                for (BackBlock &b : blocks) b.lo = 0, b.hi = index ? 0 : (uint32_t)b.size;
                BZH_TRY(back_emit(ctx, w, clock, bk, d_to, true, blocks, false, nullptr, index && rec ? &bc : nullptr));
            } else {
                span(3, bk.t_unrle);
            }
        }
        // CRCs in chain order: every block's against its header, every stream's fold against its footer
        uint32_t q = 0;
        const size_t stream_at = stream, block_at = block; // (errors below name the item they are about)
        for (const ChainItem &it : items) {
            stream = it.stream;
            block = it.block;
            if (!it.footer) {
                if ((index || !over) && blocks[q].crc != it.crc) return data_error(BZD_K_BLOCK_CRC, it.bitpos);
                if (index) {
                    if (sync) { // the points of the block's slot, numbered by the entry they belong to (the stream is idle here)
                        const uint32_t c = std::min(hptcnt[it.slot], sync_cap);
                        const size_t at = sync->pts.size();
                        sync->pts.resize(at + c);
                        if (c)
                            HIP_TRY(ctx, hipMemcpy(sync->pts.data() + at, d_pts + (size_t)it.slot * sync_cap, (size_t)c * sizeof(bzh_sync_point),
                                                   hipMemcpyDeviceToHost));
                        for (size_t p = at; p < at + c; p++) sync->pts[p].entry = (uint32_t)index->size();
                    }
                    index->push_back({it.bitpos, it.end_bit, (uint64_t)blocks[q].base, (uint32_t)blocks[q].size, it.crc, (uint32_t)it.stream, it.level});
                    if (rec) { // the tiles of the block, summed behind the entries before it
                        uint64_t d = 0;
                        for (uint32_t t = 0; t < (blocks[q].nblock + UR_TILE - 1) / UR_TILE; t++) d += bc.tcount[(size_t)it.slot * w.T + t];
                        rec->cum.push_back(rec->cum.back() + d);
                        rec->last_is_delim = bc.last[it.slot] != 0;
                    }
                }
                stream_crc = ((stream_crc << 1) | (stream_crc >> 31)) ^ it.crc;
                q++;
            } else {
                if (stream_crc != it.crc) return data_error(BZD_K_STREAM_CRC, it.bitpos);
                stream_crc = 0;
            }
        }
        stream = stream_at;
        block = block_at;
        if (sink && !blocks.empty()) BZH_TRY(sink->window(ctx, batch_bytes)); // (every block of the batch has passed its CRC)
        if (finished) break;
    }
    clock.collect();
    ds.candidates_off_chain += nc - ci; // (magics in foreign bytes behind the last stream)
    ds.out_bytes = total_out;
    *out_len = (size_t)total_out;
    if (over && !index) {
        bzh_set_error(ctx, "decode: the output needs %llu bytes, the buffer holds %zu", (unsigned long long)total_out, cap);
        return BZH_E_CAP;
    }
    return BZH_OK;
}

// ================================================================================================================
// Streaming decode (bzh_dstream_*): decode_chain_run's walk over a sliding window of the input.  The walk and the feed loop are
// decode_stream_plan.h's; this is its device: the window (two buffers -- the tail of a pass is copied from one to the front of
// the other, so no copy overlaps), the staging buffer, the scan of the appended bytes, and a pass's batch through the entropy
// stage and the back of the decoder.  No kernel of its own.  The buffers are the stream's, so between two feeds every other
// entry point may use the context; what a pass borrows of the context (decode tables, hit list, arena) it asks for anew.
// ================================================================================================================
static_assert(BZS_OK == BZH_OK && BZS_E_ARG == BZH_E_ARG && BZS_E_STATE == BZH_E_STATE && BZS_E_DATA == BZH_E_DATA,
              "decode_stream_plan.h names bzh_status values");
static_assert(sizeof(BzsStats) >= sizeof(bzh_dstream_stats) && offsetof(BzsStats, staging_peak) == offsetof(bzh_dstream_stats, staging_peak),
              "BzsStats begins with the fields of bzh_dstream_stats");
constexpr size_t DSTREAM_WINDOW = (size_t)32 << 20, DSTREAM_STAGING = (size_t)128 << 20; // the defaults bzhip.h documents
constexpr size_t DSTREAM_PAD = 16;

struct DStreamDev {
    bzh_ctx *ctx = nullptr;
    int (*arena)(bzh_ctx *, uint32_t) = nullptr;
    DevBuf win[2], staging;
    int cur = 0;
    uint64_t room = 0; // bytes the window is to hold
    DecWs w;
    Back bk;
    std::vector<uint64_t> found;
    std::vector<BackBlock> bb;

    uint32_t max_batch() const { return ctx->max_batch; }
    int win_reserve(uint64_t cap, uint64_t keep)
    {
        room = cap;
        if (win[cur].cap >= cap + DSTREAM_PAD) return BZH_OK;
        BZH_TRY(win[1 - cur].reserve(ctx, cap + DSTREAM_PAD, "the stream's window"));
        if (keep) HIP_TRY(ctx, hipMemcpyAsync(win[1 - cur], win[cur], keep, hipMemcpyDeviceToDevice, ctx->stream));
        HIP_TRY(ctx, bzh_stream_wait(ctx->stream));
        cur = 1 - cur;
        return BZH_OK;
    }
    int win_append(uint64_t at, const uint8_t *src, uint64_t n)
    {
        if (at + n > room) return BZH_E_STATE;
        HIP_TRY(ctx, hipMemcpyAsync(win[cur] + at, src, n, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, bzh_stream_wait(ctx->stream)); // (the caller's bytes are his again when the call returns)
        return BZH_OK;
    }
    int win_move(uint64_t from, uint64_t len)
    {
        if (from + len > room) return BZH_E_STATE;
        BZH_TRY(win[1 - cur].reserve(ctx, room + DSTREAM_PAD, "the stream's window"));
        HIP_TRY(ctx, hipMemcpyAsync(win[1 - cur], win[cur] + from, len, hipMemcpyDeviceToDevice, ctx->stream));
        cur = 1 - cur;
        return BZH_OK;
    }
    int scan(uint64_t from, uint64_t to, std::vector<uint64_t> &hits)
    {
        hits.clear();
        if (to > room || from > to) return BZH_E_STATE;
        BZH_TRY(decode_scan_run(ctx, win[cur] + from, to - from, found));
        for (uint64_t h : found) hits.push_back(h + (16 * from)); // (bit << 1: 8 * from bits)
        return BZH_OK;
    }
    int entropy(const uint64_t *cands, uint32_t B, uint64_t held, BzdResult *res)
    {
        hipStream_t st = ctx->stream;
        if (held > room || B == 0 || B > ctx->max_batch) return BZH_E_STATE;
        if (ctx->profiling) ctx->evnext = 0; // (the back's stage clock takes events of the pool; nobody reads them here)
        BZH_TRY(arena(ctx, B));
        if (B > ctx->arena_blocks) return BZH_E_STATE;
        BZH_TRY(dec_ws(ctx, w));
        HIP_TRY(ctx, hipMemcpyAsync(w.cand, cands, (size_t)B * 8, hipMemcpyHostToDevice, st));
        decode_block_kernel<<<dim3(B), 64, 0, st>>>(win[cur], held, w.cand, ctx->bt, w.res, 100000u * (uint32_t)ctx->level);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(res, w.res, (size_t)B * sizeof(BzdResult), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, bzh_stream_wait(st));
        return BZH_OK;
    }
    int sizes(std::vector<BzsBlock> &blocks, uint32_t Bu, uint32_t nmax_all)
    {
        StageClock clock{ctx, {}};
        bb.clear();
        for (const BzsBlock &b : blocks) bb.push_back(BackBlock{b.slot, b.nblock, 0, false, 0, 0, 0, 0});
        BZH_TRY(back_sizes(ctx, w, clock, bk, Bu, nmax_all, bb));
        for (size_t q = 0; q < blocks.size(); q++) {
            blocks[q].size = bb[q].size;
            blocks[q].bad_end = bb[q].bad_end;
        }
        return BZH_OK;
    }
    int stage_reserve(uint64_t cap) { return staging.reserve(ctx, cap + DSTREAM_PAD, "the stream's staging buffer"); }
    int emit(std::vector<BzsBlock> &blocks, size_t taken)
    {
        StageClock clock{ctx, {}};
        bb.resize(taken);
        uint64_t end = 0;
        for (size_t q = 0; q < taken; q++) {
            bb[q].base = (int64_t)blocks[q].base;
            bb[q].lo = 0;
            bb[q].hi = (uint32_t)bb[q].size;
            end = std::max(end, blocks[q].base + bb[q].size);
        }
        if (end + DSTREAM_PAD > staging.cap) return BZH_E_STATE;
        BZH_TRY(back_emit(ctx, w, clock, bk, staging, true, bb, true));
        for (size_t q = 0; q < taken; q++) blocks[q].crc = bb[q].crc;
        return BZH_OK;
    }
    int handout(uint64_t off, uint8_t *out, uint64_t n)
    {
        if (off + n + DSTREAM_PAD > staging.cap) return BZH_E_STATE;
        HIP_TRY(ctx, hipMemcpy(out, staging + off, n, hipMemcpyDeviceToHost));
        return BZH_OK;
    }
};

struct DStream {
    DStreamDev dev;
    BzsStream<DStreamDev> walk;
};

int dstream_begin(bzh_ctx *ctx)
{
    if (!ctx->dstrm) ctx->dstrm = new DStream();
    DStream &d = *ctx->dstrm;
    d.dev.ctx = ctx;
    const int rc = d.walk.begin(&d.dev, ctx->level, ctx->dstrm_window ? ctx->dstrm_window : DSTREAM_WINDOW,
                                ctx->dstrm_staging ? ctx->dstrm_staging : DSTREAM_STAGING);
    if (rc != BZH_OK) d.walk.open = false;
    return rc;
}

int dstream_feed(bzh_ctx *ctx, int (*arena)(bzh_ctx *, uint32_t), const uint8_t *in, size_t n, int eof, size_t *in_used, uint8_t *out, size_t cap,
                 size_t *out_len, int *done)
{
    *in_used = *out_len = 0;
    *done = 0;
    if (!ctx->dstrm || !ctx->dstrm->walk.open) {
        bzh_set_error(ctx, "dstream: no stream is open (no begin, or the stream has ended in an error)");
        return BZH_E_STATE;
    }
    DStream &d = *ctx->dstrm;
    d.dev.arena = arena;
    uint64_t used = 0, got = 0;
    bool fin = false;
    const int rc = d.walk.feed(in, n, eof != 0, &used, out, cap, &got, &fin);
    *in_used = (size_t)used;
    *out_len = (size_t)got;
    *done = fin ? 1 : 0;
    if (rc == BZH_OK) return rc;
    if (d.walk.open) { // a failure of the device, which has left its own text: the stream is closed all the same
        d.walk.open = false;
        return rc;
    }
    const BzsError &e = d.walk.err;
    if (rc == BZH_E_ARG)
        bzh_set_error(ctx, "decode: stream %zu is of level %u, the context of level %d", e.stream, e.level, ctx->level);
    else if (rc == BZH_E_DATA)
        bzh_set_error(ctx, "decode: %s%s%s in stream %zu, block %zu, at bit %llu", kind_name(e.kind), e.what ? ": " : "", e.what ? e.what : "",
                      e.stream, e.block, (unsigned long long)e.bit);
    else
        bzh_set_error(ctx, "dstream: %s", e.what ? e.what : "internal error");
    return rc;
}

size_t dstream_consumed(const bzh_ctx *ctx) { return ctx->dstrm ? (size_t)ctx->dstrm->walk.consumed : 0; }

int dstream_stats(const bzh_ctx *ctx, bzh_dstream_stats *out)
{
    memset(out, 0, sizeof *out);
    if (ctx->dstrm) memcpy(out, &ctx->dstrm->walk.st, sizeof *out);
    return BZH_OK;
}

void dstream_end(bzh_ctx *ctx)
{
    if (ctx->dstrm) ctx->dstrm->walk.open = false;
}

void dstream_free(bzh_ctx *ctx)
{
    delete ctx->dstrm;
    ctx->dstrm = nullptr;
}

// ================================================================================================================
// Many inputs (bzh_decode_many*): one scan, one chain per input, batches across the inputs.  The walk is decode_many_plan.h's;
// this feeds it the entropy stage's results batch by batch and runs the back of the decoder for the blocks it met.
// ================================================================================================================
static_assert(BZM_OK == BZH_OK && BZM_E_ARG == BZH_E_ARG && BZM_E_DATA == BZH_E_DATA, "decode_many_plan.h names bzh_status values");

int decode_many_run(bzh_ctx *ctx, const uint8_t *d_in, size_t n, const size_t *in_offs, const size_t *in_lens, size_t count, uint8_t *d_out,
                    size_t cap, size_t *out_offs, size_t *out_lens, int *status, size_t *consumed, const std::vector<uint64_t> &cands)
{
    static_assert(sizeof(size_t) == 8, "the slices go to the device as 64-bit words");
    hipStream_t st = ctx->stream;
    Batch &bt = ctx->bt;
    bzh_decode_stats &ds = ctx->dstats;
    bzh_decode_many_stats &ms = ctx->mstats;
    DecWs w;
    BZH_TRY(dec_ws(ctx, w));
    StageClock clock{ctx, {}};
    // the stream headers of all inputs: one launch, one copy back (no sync points in this call: their workspace is free)
    std::vector<BzmInput> ins(count);
    {
        uint64_t *d_offs, *d_lens;
        uint32_t *d_heads;
        BZH_TRY(reserve_cut(ctx, ctx->sync_ws, "the sync points", grow_mib, [&](Carver &c) { c.put(d_offs, count); c.put(d_lens, count); c.put(d_heads, count); }));
        std::vector<uint32_t> heads(count);
        HIP_TRY(ctx, hipMemcpyAsync(d_offs, in_offs, count * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(d_lens, in_lens, count * 8, hipMemcpyHostToDevice, st));
        BZH_TRY(many_heads_run(ctx, d_in, d_offs, d_lens, (uint32_t)count, d_heads));
        HIP_TRY(ctx, hipMemcpyAsync(heads.data(), d_heads, count * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, bzh_stream_wait(st));
        for (size_t k = 0; k < count; k++) {
            ins[k].off = in_offs[k];
            ins[k].len = in_lens[k];
            for (int j = 0; j < 4; j++) ins[k].head[j] = (uint8_t)(heads[k] >> (8 * j));
        }
    }
    BzmWalk walk;
    walk.cands = cands.data();
    walk.nc = cands.size();
    walk.in = ins.data();
    walk.count = count;
    walk.ctx_level = ctx->level;
    walk.start();
    const uint32_t Bmax = batch_max(ctx);
    const bool small_on = unbwt_small_enabled();
    const uint32_t small_max = (uint32_t)bzh_decode_many_small_max();
    std::vector<BzdResult> res;
    std::vector<BackBlock> blocks;
    std::vector<BzmItem *> of; // the item of every listed block
    Back bk;
    size_t first;
    uint32_t B;
    while (walk.next_batch(Bmax, &first, &B)) {
        hipEvent_t e0 = clock.mark();
        HIP_TRY(ctx, hipMemcpyAsync(w.cand, cands.data() + first, (size_t)B * 8, hipMemcpyHostToDevice, st));
        decode_block_kernel<<<dim3(B), 64, 0, st>>>(d_in, n, w.cand, bt, w.res, 100000u * (uint32_t)ctx->level);
        HIP_TRY(ctx, hipGetLastError());
        clock.span(1, e0);
        res.resize(B);
        HIP_TRY(ctx, hipMemcpyAsync(res.data(), w.res, (size_t)B * sizeof(BzdResult), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, bzh_stream_wait(st));
        ms.batches++;
        walk.feed(res.data());
        blocks.clear();
        of.clear();
        for (BzmItem &it : walk.items)
            if (!it.footer && !it.dead) {
                blocks.push_back(BackBlock{it.slot, it.nblock, 0, false, 0, 0, 0, 0});
                of.push_back(&it);
            }
        if (!blocks.empty()) {
            // (the inverse BWT runs over slots: the clean candidates off the chain among them set its size too)
            auto nmax_upto = [&](uint32_t Bu) {
                uint32_t m = 1;
                for (uint32_t s = 0; s < Bu; s++)
                    if (!(cands[first + s] & 1ull) && res[s].kind == BZD_OK) m = std::max(m, res[s].nblock);
                return m;
            };
            const uint32_t Bu = blocks.back().slot + 1;
            if (small_on) {
                BackSplit split{small_max, 0, 1, 0};
                for (const BackBlock &b : blocks)
                    if (b.nblock > small_max) split.Bl = b.slot + 1;
                split.nmax_l = nmax_upto(split.Bl);
                BZH_TRY(back_sizes(ctx, w, clock, bk, Bu, 0, blocks, &split));
                ms.blocks_small += split.nsmall;
            } else {
                BZH_TRY(back_sizes(ctx, w, clock, bk, Bu, nmax_upto(Bu), blocks));
            }
            for (size_t q = 0; q < blocks.size(); q++) {
                of[q]->size = blocks[q].size;
                of[q]->bad_end = blocks[q].bad_end;
            }
        }
        walk.place(cap);
        if (!blocks.empty()) {
            if (!walk.over) { // a block of an input that has failed by now is not written (an empty window)
                for (size_t q = 0; q < blocks.size(); q++) {
                    blocks[q].base = (int64_t)of[q]->base;
                    blocks[q].lo = 0;
                    blocks[q].hi = of[q]->placed ? (uint32_t)blocks[q].size : 0;
                }
                BZH_TRY(back_emit(ctx, w, clock, bk, d_out, true, blocks));
                for (size_t q = 0; q < blocks.size(); q++) of[q]->got_crc = blocks[q].crc;
            } else {
                clock.span(3, bk.t_unrle);
            }
        }
        walk.check(!walk.over);
    }
    walk.finish();
    clock.collect();
    ds.candidates_off_chain = walk.off_chain;
    ds.streams = walk.streams;
    ds.blocks = walk.blocks;
    ds.out_bytes = walk.total_out;
    ms.inputs = count;
    ms.inputs_failed = walk.failed;
    ms.streams = walk.streams;
    ms.blocks = walk.blocks;
    bool named = false;
    for (size_t k = 0; k < count; k++) {
        const BzmState &s = walk.st[k];
        out_offs[k] = (size_t)s.out_off;
        out_lens[k] = (size_t)s.out_len;
        status[k] = s.status;
        if (consumed) consumed[k] = (size_t)s.consumed;
        if (s.status == BZH_OK || named) continue;
        named = true;
        const BzmError &e = s.err;
        if (e.kind == BZD_OK)
            bzh_set_error(ctx, "decode: input %zu: stream %zu is of level %u, the context of level %d", k, e.stream, e.level, ctx->level);
        else
            bzh_set_error(ctx, "decode: input %zu: %s%s%s in stream %zu, block %zu, at bit %llu", k, kind_name(e.kind), e.what ? ": " : "",
                          e.what ? e.what : "", e.stream, e.block, (unsigned long long)e.bit);
    }
    if (walk.over) {
        bzh_set_error(ctx, "decode: the output needs %llu bytes, the buffer holds %zu", (unsigned long long)walk.total_out, cap);
        return BZH_E_CAP;
    }
    return BZH_OK;
}

// ================================================================================================================
// Recovery (bzh_recover*): every block magic judged on its own.  The walk is decode_recover_plan.h's; this feeds it the entropy
// stage's results batch by batch, the sizes of the clean candidates and -- the verdict before the placement -- their CRCs folded
// from the bytes behind the inverse BWT (an empty window: unrle_crc), and then expands the blocks it kept where they belong.
// ================================================================================================================
int decode_recover_run(bzh_ctx *ctx, const uint8_t *d_in, size_t n, uint8_t *d_out, size_t cap, size_t *out_len,
                       std::vector<bzh_recover_entry> &entries, bzh_recover_stats &stats, const std::vector<uint64_t> &cands)
{
    hipStream_t st = ctx->stream;
    Batch &bt = ctx->bt;
    DecWs w;
    BZH_TRY(dec_ws(ctx, w));
    StageClock clock{ctx, {}};
    BzrWalk walk;
    walk.cands = cands.data();
    walk.nc = cands.size();
    walk.n = n;
    walk.ctx_level = ctx->level;
    if (n) HIP_TRY(ctx, hipMemcpyAsync(walk.head, d_in, std::min<size_t>(n, 4), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, bzh_stream_wait(st));
    walk.start();
    const uint32_t Bmax = batch_max(ctx);
    std::vector<BzdResult> res;
    std::vector<BackBlock> blocks, sub;
    std::vector<size_t> sub_of; // the block of every listed one
    Back bk;
    size_t first;
    uint32_t B;
    while (walk.next_batch(Bmax, &first, &B)) {
        hipEvent_t e0 = clock.mark();
        HIP_TRY(ctx, hipMemcpyAsync(w.cand, cands.data() + first, (size_t)B * 8, hipMemcpyHostToDevice, st));
        decode_block_kernel<<<dim3(B), 64, 0, st>>>(d_in, n, w.cand, bt, w.res, 100000u * (uint32_t)ctx->level);
        HIP_TRY(ctx, hipGetLastError());
        clock.span(1, e0);
        res.resize(B);
        HIP_TRY(ctx, hipMemcpyAsync(res.data(), w.res, (size_t)B * sizeof(BzdResult), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, bzh_stream_wait(st));
        walk.feed(res.data());
        blocks.clear();
        for (const BzrItem &it : walk.items) blocks.push_back(BackBlock{it.slot, it.nblock, 0, false, 0, 0, 0, 0});
        if (!blocks.empty()) {
            const uint32_t Bu = blocks.back().slot + 1;
            uint32_t nmax_all = 1; // (the inverse BWT runs over slots: every clean candidate among them sets its size)
            for (uint32_t s = 0; s < Bu; s++)
                if (!(cands[first + s] & 1ull) && res[s].kind == BZD_OK) nmax_all = std::max(nmax_all, res[s].nblock);
            BZH_TRY(back_sizes(ctx, w, clock, bk, Bu, nmax_all, blocks));
            // the verdict: the CRC of every block that does not end in four equal bytes without a count, nothing written
            sub.clear(), sub_of.clear();
            for (size_t q = 0; q < blocks.size(); q++) {
                walk.items[q].size = blocks[q].size;
                walk.items[q].bad_end = blocks[q].bad_end;
                if (blocks[q].bad_end) continue;
                sub.push_back(blocks[q]); // (lo == hi == 0: the empty window)
                sub_of.push_back(q);
            }
            if (!sub.empty()) {
                BZH_TRY(back_emit(ctx, w, clock, bk, nullptr, true, sub));
                for (size_t q = 0; q < sub.size(); q++) walk.items[sub_of[q]].got_crc = sub[q].crc;
            } else {
                clock.span(3, bk.t_unrle);
            }
        }
        walk.select();
        walk.place(cap);
        if (!walk.over) { // the placement: the kept blocks, whole
            sub.clear();
            for (size_t q = 0; q < blocks.size(); q++) {
                if (!walk.items[q].kept) continue;
                BackBlock b = blocks[q];
                b.base = (int64_t)walk.items[q].base;
                b.lo = 0;
                b.hi = (uint32_t)b.size;
                sub.push_back(b);
            }
            if (!sub.empty()) {
                bk.t_unrle = clock.mark();
                BZH_TRY(back_emit(ctx, w, clock, bk, d_out, false, sub, true));
            }
        }
    }
    walk.finish();
    clock.collect();
    entries.swap(walk.entries);
    stats = walk.stats;
    *out_len = (size_t)walk.total_out;
    if (walk.over) {
        bzh_set_error(ctx, "recover: the output needs %llu bytes, the buffer holds %zu", (unsigned long long)walk.total_out, cap);
        return BZH_E_CAP;
    }
    return BZH_OK;
}

// first_bad: the first of the `count` bit positions at which no block magic stands (count: every one holds one)
int decode_magic_run(bzh_ctx *ctx, const uint8_t *d_in, size_t n, const uint64_t *pos, size_t count, size_t *first_bad)
{
    hipStream_t st = ctx->stream;
    *first_bad = count;
    if (count == 0) return BZH_OK;
    uint64_t *d_cand = nullptr;
    uint32_t *d_bad = nullptr;
    BZH_TRY(reserve_cut(ctx, ctx->sync_ws, "the sync points", grow_mib, [&](Carver &c) { c.put(d_cand, count); c.put(d_bad, count); }));
    std::vector<uint64_t> hc(count);
    for (size_t k = 0; k < count; k++) hc[k] = pos[k] << 1;
    std::vector<uint32_t> hbad(count);
    HIP_TRY(ctx, hipMemcpyAsync(d_cand, hc.data(), count * 8, hipMemcpyHostToDevice, st));
    range_magic_kernel<<<dim3((uint32_t)((count + 63) / 64)), 64, 0, st>>>(d_in, n, d_cand, (uint32_t)count, d_bad);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(hbad.data(), d_bad, count * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, bzh_stream_wait(st));
    for (size_t k = 0; k < count; k++)
        if (hbad[k]) {
            *first_bad = k;
            break;
        }
    return BZH_OK;
}

// ================================================================================================================
// Random access: bzh_index_span, and the decode of the blocks a range touches (bzh_decode_range*)
// ================================================================================================================
// The entries [*first, *last) that [off, off + len) touches, *clipped = min(len, total - off), and the bytes of the indexed input
// that hold them.  Offsets ascend, so both ends are binary searches.
static void index_span(const bzh_index_entry *idx, size_t count, uint64_t off, uint64_t len, size_t *first, size_t *last,
                       uint64_t *byte_lo, uint64_t *byte_hi, uint64_t *clipped)
{
    const uint64_t total = count ? idx[count - 1].out_off + idx[count - 1].out_len : 0;
    *clipped = off < total ? std::min<uint64_t>(len, total - off) : 0;
    // the first entry that ends behind `off`
    size_t lo = 0, hi = count;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (idx[mid].out_off + idx[mid].out_len <= off)
            lo = mid + 1;
        else
            hi = mid;
    }
    *first = *last = lo;
    *byte_lo = *byte_hi = 0;
    if (*clipped == 0) return;
    const uint64_t end = off + *clipped; // the first entry that starts at or behind the end of the range
    hi = count;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (idx[mid].out_off < end)
            lo = mid + 1;
        else
            hi = mid;
    }
    *last = lo;
    if (*last <= *first) { // (only an index whose offsets are not the running sum from 0 gets here: no entry holds the range)
        *last = *first;
        return;
    }
    *byte_lo = idx[*first].bit_pos / 8;
    *byte_hi = (idx[*last - 1].end_bit + 7) / 8;
}

extern "C" int bzh_index_span(const bzh_index_entry *idx, size_t count, uint64_t off, uint64_t len, size_t *first, size_t *last,
                              uint64_t *byte_lo, uint64_t *byte_hi)
{
    if ((!idx && count) || !first || !last || !byte_lo || !byte_hi) return BZH_E_ARG;
    uint64_t clipped;
    index_span(idx, count, off, len, first, last, byte_lo, byte_hi, &clipped);
    return BZH_OK;
}

// The index, well formed as a whole, whatever the range: BZH_E_ARG naming the first entry that is not.  Both entry points call
// this before any arithmetic on the entries.
int decode_index_check(bzh_ctx *ctx, const bzh_index_entry *idx, size_t count)
{
    uint64_t sum = 0;
    for (size_t k = 0; k < count; k++) {
        const bzh_index_entry &e = idx[k];
        const char *what = nullptr;
        if (e.end_bit <= e.bit_pos)
            what = "end_bit is not behind bit_pos";
        else if (k && e.bit_pos <= idx[k - 1].bit_pos)
            what = "bit_pos does not ascend";
        else if (e.out_off != sum)
            what = "out_off is not the running sum of the sizes before it";
        else if (e.level < 1 || e.level > 9)
            what = "a level outside 1..9";
        else if ((int)e.level > ctx->level)
            what = "a level above the context's";
        if (what) {
            bzh_set_error(ctx, "decode range: index entry %zu: %s", k, what);
            return BZH_E_ARG;
        }
        sum += e.out_len;
    }
    return BZH_OK;
}

// The sync points, well formed as a whole against the index (which has passed decode_index_check), whatever the range: BZH_E_ARG
// naming the first point that is not.  The rule itself is decode_core.h's, shared with the host model.
int decode_sync_check(bzh_ctx *ctx, const bzh_index_entry *idx, size_t count, const bzh_sync_point *pts, size_t npts)
{
    for (size_t i = 0; i < npts; i++) {
        const char *what = bzd_sync_point_check(idx, count, pts, i);
        if (what) {
            bzh_set_error(ctx, "decode range: sync point %zu: %s", i, what);
            return BZH_E_ARG;
        }
    }
    return BZH_OK;
}

// The entries first .. last that a read touches lie in the buffer: n bytes of the indexed input from byte in_byte_base on.
static int index_covered(bzh_ctx *ctx, const bzh_index_entry *idx, size_t first, size_t last, uint64_t in_byte_base, size_t n)
{
    const uint64_t byte_lo = idx[first].bit_pos / 8, byte_hi = (idx[last].end_bit + 7) / 8;
    if (in_byte_base <= byte_lo && byte_hi - in_byte_base <= n) return BZH_OK;
    bzh_set_error(ctx, "decode range: index entries %zu..%zu lie in bytes [%llu, %llu) of the indexed input, the buffer holds [%llu, %llu)",
                  first, last, (unsigned long long)byte_lo, (unsigned long long)byte_hi, (unsigned long long)in_byte_base,
                  (unsigned long long)(in_byte_base + n));
    return BZH_E_ARG;
}

// The front of a batch of every read by index (decode_range_run, decode_ranges_run, decode_records_run): the entropy stage of the
// entries idx[ent[0 .. B)] -- ascending, block k in batch slot k --, every block checked against its entry, then back_sizes and the
// sizes checked too.  BZH_E_DATA names the first entry that fails, and a sync point by its number in pts.  count: back_sizes' (null:
// none).  The caller sets the blocks' windows (or asks `pieces` for them), calls back_emit and then `crcs`.
struct IndexedFront {
    bzh_ctx *ctx;
    const DecWs &w;
    StageClock &clock;
    const uint8_t *d_in;
    size_t n;
    uint64_t in_byte_base;
    const bzh_index_entry *idx;
    const bzh_sync_point *pts;
    size_t npts;
    size_t at = 0;        // the entry an error is about
    size_t seg_point = 0; // the sync point a segment's error is about
    std::vector<SegDesc> hseg;
    std::vector<BzdSegResult> hsres;
    std::vector<uint32_t> seg0; // [B + 1] first segment of every block of the batch
    std::vector<size_t> pmap;   // the batch's points, gathered: which of pts each is
    std::vector<bzh_sync_point> hpts;
    std::vector<uint64_t> hcand;
    std::vector<BzdResult> res;
    std::vector<uint32_t> hmagic;
    std::vector<BackBlock> blocks;
    Back bk;

    int mismatch(const char *what)
    {
        bzh_set_error(ctx, "decode range: index entry %zu (stream %u, bit %llu) does not match its block: %s", at, idx[at].stream,
                      (unsigned long long)idx[at].bit_pos, what);
        return BZH_E_DATA;
    }
    int seg_mismatch(bool named, const char *what)
    {
        if (!named) return mismatch(what);
        bzh_set_error(ctx, "decode range: index entry %zu (stream %u, bit %llu) does not match its block: sync point %zu: %s", at, idx[at].stream,
                      (unsigned long long)idx[at].bit_pos, seg_point, what);
        return BZH_E_DATA;
    }
    int run(const uint32_t *ent, uint32_t B, BackCount *count = nullptr)
    {
        hipStream_t st = ctx->stream;
        Batch &bt = ctx->bt;
        // entropy stage: the entries are the candidates
        hcand.resize(B);
        for (uint32_t k = 0; k < B; k++) hcand[k] = (idx[ent[k]].bit_pos - 8 * in_byte_base) << 1;
        BzdHead *d_heads = nullptr;
        bzh_sync_point *d_pts = nullptr;
        SegDesc *d_segs = nullptr;
        BzdSegResult *d_sres = nullptr;
        if (npts) {
            bzp_segments(idx, ent, B, pts, npts, hseg, seg0, pmap);
            hpts.resize(pmap.size());
            for (size_t j = 0; j < pmap.size(); j++) hpts[j] = pts[pmap[j]];
            BZH_TRY(reserve_cut(ctx, ctx->sync_ws, "the sync points", grow_mib, [&](Carver &c) { // (the stream is idle between batches)
                c.put(d_heads, B), c.put(d_pts, hpts.size());
                c.put(d_segs, hseg.size()), c.put(d_sres, hseg.size());
            }));
        }
        hipEvent_t t1 = clock.mark();
        HIP_TRY(ctx, hipMemcpyAsync(w.cand, hcand.data(), (size_t)B * 8, hipMemcpyHostToDevice, st));
        if (npts) {
            if (!hpts.empty()) HIP_TRY(ctx, hipMemcpyAsync(d_pts, hpts.data(), hpts.size() * sizeof(bzh_sync_point), hipMemcpyHostToDevice, st));
            HIP_TRY(ctx, hipMemcpyAsync(d_segs, hseg.data(), hseg.size() * sizeof(SegDesc), hipMemcpyHostToDevice, st));
            decode_header_kernel<<<dim3(B), 64, 0, st>>>(d_in, n, w.cand, d_heads, w.res);
            decode_segment_kernel<<<dim3((uint32_t)hseg.size()), 64, 0, st>>>(d_in, n, 8 * in_byte_base, d_heads, d_pts, d_segs, bt, w.res, d_sres);
        } else {
            decode_block_kernel<<<dim3(B), 64, 0, st>>>(d_in, n, w.cand, bt, w.res, 100000u * (uint32_t)ctx->level);
        }
        range_magic_kernel<<<dim3((B + 63) / 64), 64, 0, st>>>(d_in, n, w.cand, B, w.magic);
        HIP_TRY(ctx, hipGetLastError());
        clock.span(1, t1);
        res.resize(B);
        hmagic.resize(B);
        if (npts) {
            hsres.resize(hseg.size());
            HIP_TRY(ctx, hipMemcpyAsync(hsres.data(), d_sres, hseg.size() * sizeof(BzdSegResult), hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(ctx, hipMemcpyAsync(res.data(), w.res, (size_t)B * sizeof(BzdResult), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(hmagic.data(), w.magic, (size_t)B * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, bzh_stream_wait(st));
        uint32_t nmax = 1;
        for (uint32_t k = 0; k < B; k++) {
            at = ent[k];
            const bzh_index_entry &e = idx[at];
            BzdResult &r = res[k];
            if (hmagic[k]) return mismatch("no block magic at bit_pos");
            if (r.kind != BZD_OK) return mismatch(kind_name(r.kind));
            if (npts) { // every segment in order: the first that fails names the point it could not start from or arrive at
                for (uint32_t g = seg0[k]; g < seg0[k + 1]; g++) {
                    const BzdSegResult &sr = hsres[g];
                    const SegDesc &d = hseg[g];
                    const bool named = d.from >= 0 || d.to >= 0;
                    if (sr.miss == BZD_SEG_START) {
                        if (named) seg_point = pmap[(size_t)(d.from >= 0 ? d.from : d.to)];
                        return seg_mismatch(named, "it is no state of this block");
                    }
                    if (named) seg_point = pmap[(size_t)(d.to >= 0 ? d.to : d.from)];
                    if (sr.kind != BZD_OK) return seg_mismatch(named, kind_name(sr.kind));
                    if (sr.miss == BZD_SEG_EOB) return seg_mismatch(named, "the block ends in front of it");
                    if (sr.miss == BZD_SEG_ARRIVE) return seg_mismatch(named, "the segment in front of it arrives in another state");
                    if (d.to < 0) {
                        r.end_bit = sr.end_bit;
                        r.nblock = sr.nblock;
                    }
                }
            }
            if (r.end_bit + 8 * in_byte_base != e.end_bit) return mismatch("it ends at another bit than end_bit");
            if (r.crc != e.crc) return mismatch("its stored CRC differs");
            if (r.nblock > 100000u * e.level) return mismatch("more bytes than the level's block size");
            nmax = std::max(nmax, r.nblock);
        }
        ctx->dstats.blocks += B;
        blocks.clear();
        for (uint32_t k = 0; k < B; k++) blocks.push_back(BackBlock{k, res[k].nblock, 0, false, 0, 0, 0, 0});
        BZH_TRY(back_sizes(ctx, w, clock, bk, B, nmax, blocks, nullptr, count));
        for (uint32_t k = 0; k < B; k++) {
            at = ent[k];
            if (blocks[k].bad_end) return mismatch("the block ends in four equal bytes without a count");
            if (blocks[k].size != idx[at].out_len) return mismatch("it decodes to another size than out_len");
        }
        return BZH_OK;
    }
    // The windows of the batch's blocks for back_emit, from their pieces: block k wants pc[pfirst[k] .. pfirst[k + 1]), each somewhere
    // in an output of out_total bytes.
    std::vector<uint32_t> pslots, ptiles, tile_first;
    std::vector<size_t> pf;     // the pieces of the batch's blocks that are emitted piece by piece: bpc[pf[k] .. pf[k + 1])
    std::vector<PieceRef> bpc, refs;
    int pieces(const size_t *pfirst, const std::vector<PieceRef> &pc, uint32_t B, uint64_t out_total, BackPieces &bp, uint64_t *whole)
    {
        // A block that one range wants whole and no other touches is expanded where it belongs and checked there; every other one
        // goes out piece by piece, its window here empty: back_emit takes its CRC from the bytes behind the inverse BWT.
        pslots.clear(), ptiles.clear(), bpc.clear();
        pf.assign(1, 0);
        for (uint32_t k = 0; k < B; k++) {
            const uint32_t out_len = (uint32_t)blocks[k].size; // (== its entry's: run has checked)
            BackBlock &b = blocks[k];
            const size_t q0 = pfirst[k], q1 = pfirst[k + 1];
            if (q1 - q0 == 1 && pc[q0].lo == 0 && pc[q0].hi == out_len) {
                b.hi = out_len;
                b.base = (int64_t)pc[q0].base;
                (*whole)++;
                continue;
            }
            pslots.push_back(k);
            ptiles.push_back((b.nblock + UR_TILE - 1) / UR_TILE);
            bpc.insert(bpc.end(), pc.begin() + q0, pc.begin() + q1);
            pf.push_back(bpc.size());
        }
        bp = BackPieces{nullptr, (uint32_t)pslots.size(), UpArgs{nullptr, nullptr, bk.Tn, 0, out_total}};
        if (bp.K) {
            if (!bzp_pieces(pslots.data(), ptiles.data(), bp.K, bk.hout.data(), bk.hoff.data(), w.T, bk.Tn, pf.data(), bpc.data(), tile_first,
                            refs)) {
                bzh_set_error(ctx, "decode ranges: the ranges meet the tiles of one batch more than 2^32 times");
                return BZH_E_ARG;
            }
            hipStream_t st = ctx->stream;
            uint32_t *d_slots = nullptr, *d_first = nullptr;
            PieceRef *d_refs = nullptr;
            BZH_TRY(reserve_cut(ctx, ctx->ranges_ws, "the pieces of the ranges", grow_mib, [&](Carver &c) {
                c.put(d_refs, refs.size()), c.put(d_first, tile_first.size()), c.put(d_slots, bp.K);
            }));
            HIP_TRY(ctx, hipMemcpyAsync(d_slots, pslots.data(), (size_t)bp.K * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(ctx, hipMemcpyAsync(d_first, tile_first.data(), tile_first.size() * 4, hipMemcpyHostToDevice, st));
            if (!refs.empty()) HIP_TRY(ctx, hipMemcpyAsync(d_refs, refs.data(), refs.size() * sizeof(PieceRef), hipMemcpyHostToDevice, st));
            bp.slots = d_slots;
            bp.args.tile_first = d_first;
            bp.args.refs = d_refs;
            bp.args.nrefs = (uint32_t)refs.size();
        }
        return BZH_OK;
    }
    // behind back_emit: every block's CRC against its entry's, the first entry that fails named -- ascending, or (whole_first: the
    // single range) the whole blocks in front of the cut ones
    int crcs(const uint32_t *ent, uint32_t B, bool whole_first = false)
    {
        for (int cut = 0; cut < (whole_first ? 2 : 1); cut++)
            for (uint32_t k = 0; k < B; k++) {
                if ((whole_first && blocks[k].whole() != (cut == 0)) || blocks[k].crc == idx[ent[k]].crc) continue;
                at = ent[k];
                return mismatch(kind_name(BZD_K_BLOCK_CRC));
            }
        return BZH_OK;
    }
};

// (idx has passed decode_index_check -- a range that holds bytes touches an entry --, pts decode_sync_check; count < 2^32)
int decode_range_run(bzh_ctx *ctx, const uint8_t *d_in, size_t n, uint64_t in_byte_base, const bzh_index_entry *idx, size_t count,
                     uint64_t off, uint64_t len, uint8_t *d_out, size_t cap, size_t *out_len, const bzh_sync_point *pts, size_t npts)
{
    bzh_decode_stats &ds = ctx->dstats;
    *out_len = 0;
    size_t first, last;
    uint64_t byte_lo, byte_hi, clipped;
    index_span(idx, count, off, len, &first, &last, &byte_lo, &byte_hi, &clipped);
    if (clipped == 0) return BZH_OK;
    if (clipped > cap) {
        bzh_set_error(ctx, "decode range: the range holds %llu bytes, the buffer %zu", (unsigned long long)clipped, cap);
        return BZH_E_ARG;
    }
    BZH_TRY(index_covered(ctx, idx, first, last - 1, in_byte_base, n));
    DecWs w;
    BZH_TRY(dec_ws(ctx, w));
    StageClock clock{ctx, {}};
    const uint32_t Bmax = batch_max(ctx);
    const uint64_t end = off + clipped;
    std::vector<uint32_t> touched(last - first); // first .. last - 1
    for (size_t t = 0; t < touched.size(); t++) touched[t] = (uint32_t)(first + t);
    IndexedFront fr{ctx, w, clock, d_in, n, in_byte_base, idx, pts, npts};
    for (size_t t0 = 0; t0 < touched.size();) {
        const uint32_t B = (uint32_t)std::min<size_t>(Bmax, touched.size() - t0);
        const uint32_t *ent = touched.data() + t0;
        BZH_TRY(fr.run(ent, B));
        for (uint32_t k = 0; k < B; k++) {
            // the window of the range inside this block; a block wholly inside is expanded where it belongs and checked there
            const bzh_index_entry &e = idx[ent[k]];
            BackBlock &b = fr.blocks[k];
            bzp_window(e.out_off, e.out_len, off, end, &b.lo, &b.hi);
            b.base = (int64_t)e.out_off - (int64_t)off;
        }
        BZH_TRY(back_emit(ctx, w, clock, fr.bk, d_out, true, fr.blocks));
        BZH_TRY(fr.crcs(ent, B, true));
        t0 += B;
    }
    clock.collect();
    ds.out_bytes = clipped;
    *out_len = (size_t)clipped;
    return BZH_OK;
}

// ================================================================================================================
// Many ranges in one call (bzh_decode_ranges*): the front over the union of the ranges' entries, each block decoded once
// ================================================================================================================
extern "C" int bzh_index_spans(const bzh_index_entry *idx, size_t count, const bzh_range *ranges, size_t nranges, uint32_t *touched,
                               size_t max, size_t *ntouched, uint64_t *byte_lo, uint64_t *byte_hi, uint64_t *out_total)
{
    if ((!idx && count) || (!ranges && nranges) || (!touched && max) || !ntouched || !byte_lo || !byte_hi || !out_total) return BZH_E_ARG;
    if (count > 0xFFFFFFFFull) return BZH_E_ARG;
    std::vector<uint32_t> list;
    *out_total = bzp_spans(idx, count, ranges, nranges, nullptr, nullptr, list, byte_lo, byte_hi);
    *ntouched = list.size();
    if (list.size() > max) return BZH_E_CAP;
    if (!list.empty()) memcpy(touched, list.data(), list.size() * sizeof(uint32_t));
    return BZH_OK;
}

#ifdef BZH_EXPERIMENTS
// scripts/gpu_ranges.py: the pieces of a batch (IndexedFront::pieces has listed them) through unrle_walk_win, a grid row each, to
// set beside unrle_walk_pieces.  Behind back_emit, which was given no pieces; one wait more.
static int pieces_by_window(bzh_ctx *ctx, const IndexedFront &fr)
{
    hipStream_t st = ctx->stream;
    std::vector<uint32_t> xs, xlo, xhi;
    std::vector<int64_t> xbase;
    for (size_t k = 0; k + 1 < fr.pf.size(); k++)
        for (size_t q = fr.pf[k]; q < fr.pf[k + 1]; q++) {
            xs.push_back(fr.pslots[k]), xlo.push_back(fr.bpc[q].lo), xhi.push_back(fr.bpc[q].hi);
            xbase.push_back((int64_t)fr.bpc[q].base - (int64_t)fr.bpc[q].lo);
        }
    const uint32_t P = (uint32_t)fr.bpc.size();
    if (!P) return BZH_OK;
    uint32_t *d_xs = nullptr, *d_xlo = nullptr, *d_xhi = nullptr;
    int64_t *d_xbase = nullptr;
    BZH_TRY(reserve_cut(ctx, ctx->ranges_ws, "the pieces of the ranges", grow_mib,
                        [&](Carver &c) { c.put(d_xbase, P), c.put(d_xs, P), c.put(d_xlo, P), c.put(d_xhi, P); }));
    HIP_TRY(ctx, hipMemcpyAsync(d_xs, xs.data(), (size_t)P * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_xlo, xlo.data(), (size_t)P * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_xhi, xhi.data(), (size_t)P * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(d_xbase, xbase.data(), (size_t)P * 8, hipMemcpyHostToDevice, st));
    UrArgs ax = fr.bk.a; // (out: back_emit has set it)
    ax.slots = d_xs;
    unrle_walk_win<<<dim3(fr.bk.Tn, P), UR_THREADS, 0, st>>>(ax, UwArgs{d_xlo, d_xhi, d_xbase, nullptr, nullptr, nullptr, nullptr});
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, bzh_stream_wait(st));
    return BZH_OK;
}
#endif

// back_emit for a batch of decode_ranges_run.  A build with BZH_EXPERIMENTS sends the pieces through pieces_by_window instead
// where BZH_RANGES_WIN is set.
static int ranges_emit(bzh_ctx *ctx, const DecWs &w, StageClock &clock, IndexedFront &fr, uint8_t *d_out, BackPieces &bp)
{
#ifdef BZH_EXPERIMENTS
    if (bp.K && getenv("BZH_RANGES_WIN")) {
        bp.K = 0;
        BZH_TRY(back_emit(ctx, w, clock, fr.bk, d_out, true, fr.blocks, false, &bp));
        return pieces_by_window(ctx, fr);
    }
#endif
    return back_emit(ctx, w, clock, fr.bk, d_out, true, fr.blocks, false, &bp);
}

// (idx has passed decode_index_check, pts decode_sync_check; touched and out_offs are bzp_spans', whose sum is out_total <= the
// room at d_out)
int decode_ranges_run(bzh_ctx *ctx, const uint8_t *d_in, size_t n, uint64_t in_byte_base, const bzh_index_entry *idx, size_t count,
                      const bzh_sync_point *pts, size_t npts, const bzh_range *ranges, size_t nranges, const size_t *out_offs,
                      const std::vector<uint32_t> &touched, uint8_t *d_out, uint64_t out_total)
{
    bzh_decode_stats &ds = ctx->dstats;
    bzh_decode_ranges_stats &qs = ctx->qstats;
    if (touched.empty()) return BZH_OK;
    BZH_TRY(index_covered(ctx, idx, touched.front(), touched.back(), in_byte_base, n));
    DecWs w;
    BZH_TRY(dec_ws(ctx, w));
    // what every range wants of every touched block
    std::vector<size_t> pfirst;
    std::vector<PieceRef> pc;
    std::vector<uint32_t> prange;
    bzp_block_pieces(idx, count, ranges, nranges, out_offs, touched, pfirst, pc, prange);
    qs.pieces = pc.size();
    StageClock clock{ctx, {}};
    const uint32_t Bmax = batch_max(ctx);
    IndexedFront fr{ctx, w, clock, d_in, n, in_byte_base, idx, pts, npts};
    for (size_t t0 = 0; t0 < touched.size();) {
        const uint32_t B = (uint32_t)std::min<size_t>(Bmax, touched.size() - t0);
        const uint32_t *ent = touched.data() + t0;
        qs.batches++;
        BZH_TRY(fr.run(ent, B));
        BackPieces bp;
        BZH_TRY(fr.pieces(pfirst.data() + t0, pc, B, out_total, bp, &qs.blocks_whole));
        BZH_TRY(ranges_emit(ctx, w, clock, fr, d_out, bp));
        BZH_TRY(fr.crcs(ent, B));
        t0 += B;
    }
    clock.collect();
    ds.out_bytes = out_total;
    return BZH_OK;
}

// ================================================================================================================
// Reads by record number (bzh_record_spans, bzh_decode_records*, bzh_count_records_device); the arithmetic: decode_records_plan.h
// ================================================================================================================
extern "C" int bzh_record_spans(const bzh_index_entry *idx, size_t count, const uint64_t *rec_cum, const bzh_range *ranges, size_t nranges,
                                uint32_t *touched, size_t max, size_t *ntouched, uint64_t *byte_lo, uint64_t *byte_hi)
{
    if ((!idx && count) || !rec_cum || (!ranges && nranges) || (!touched && max) || !ntouched || !byte_lo || !byte_hi) return BZH_E_ARG;
    if (count > 0xFFFFFFFFull) return BZH_E_ARG;
    size_t bad;
    if (bzq_table_check(idx, count, rec_cum, &bad)) return BZH_E_ARG;
    std::vector<uint32_t> list;
    bzq_spans(idx, count, rec_cum, ranges, nranges, list, byte_lo, byte_hi);
    *ntouched = list.size();
    if (list.size() > max) return BZH_E_CAP;
    if (!list.empty()) memcpy(touched, list.data(), list.size() * sizeof(uint32_t));
    return BZH_OK;
}

// (idx has passed decode_index_check, pts decode_sync_check, rec_cum bzq_table_check; touched is bzq_spans' list)
int decode_records_run(bzh_ctx *ctx, const uint8_t *d_in, size_t n, uint64_t in_byte_base, const bzh_index_entry *idx, size_t count,
                       const bzh_sync_point *pts, size_t npts, const uint64_t *rec_cum, uint8_t delim, const bzh_range *ranges, size_t nranges,
                       const std::vector<uint32_t> &touched, uint8_t *d_out, size_t cap, size_t *out_offs, size_t *out_lens, size_t *out_total)
{
    hipStream_t st = ctx->stream;
    bzh_decode_stats &ds = ctx->dstats;
    bzh_decode_ranges_stats &qs = ctx->qstats;
    BzqWalk<bzh_index_entry, bzh_range> walk;
    size_t bad = 0;
    if (!walk.start(idx, count, rec_cum, ranges, nranges, &bad)) {
        bzh_set_error(ctx, "decode records: range %zu begins in front of the end of the range before it", bad);
        return BZH_E_ARG;
    }
    bool over = false;
    if (!touched.empty()) {
        BZH_TRY(index_covered(ctx, idx, touched.front(), touched.back(), in_byte_base, n));
        DecWs w;
        BZH_TRY(dec_ws(ctx, w));
        BackCount bc{delim, nullptr, nullptr, {}, {}};
        BzqQuery *d_q = nullptr;
        uint32_t *d_pos = nullptr;
        BZH_TRY(back_count_ws(ctx, bc, walk.bounds.size(), &d_q, &d_pos));
        StageClock clock{ctx, {}};
        const uint32_t Bmax = batch_max(ctx);
        IndexedFront fr{ctx, w, clock, d_in, n, in_byte_base, idx, pts, npts};
        std::vector<uint32_t> ntiles, hpos;
        std::vector<BzqQuery> hq;
        std::vector<size_t> pfirst;
        std::vector<PieceRef> pc;
        auto table_mismatch = [&]() {
            bzh_set_error(ctx, "decode records: the record table does not match entry %zu", bad);
            return BZH_E_DATA;
        };
        for (size_t t0 = 0; t0 < touched.size();) {
            const uint32_t B = (uint32_t)std::min<size_t>(Bmax, touched.size() - t0);
            const uint32_t *ent = touched.data() + t0;
            qs.batches++;
            BZH_TRY(fr.run(ent, B, &bc)); // (the delimiters of every tile come back with the sizes: no wait of their own)
            ntiles.resize(B);
            for (uint32_t k = 0; k < B; k++) ntiles[k] = (fr.blocks[k].nblock + UR_TILE - 1) / UR_TILE;
            if (!walk.queries(ent, B, bc.tcount.data(), w.T, ntiles.data(), hq, &bad)) return table_mismatch();
            hpos.assign(hq.size(), BZQ_NONE);
            if (!hq.empty()) { // the boundary delimiters of this batch: the one wait a read by bytes does not pay
                HIP_TRY(ctx, hipMemcpyAsync(w.toff, fr.bk.hoff.data(), fr.bk.hoff.size() * 4, hipMemcpyHostToDevice, st));
                HIP_TRY(ctx, hipMemcpyAsync(d_q, hq.data(), hq.size() * sizeof(BzqQuery), hipMemcpyHostToDevice, st));
                unrle_select<<<dim3((uint32_t)hq.size()), UR_THREADS, 0, st>>>(fr.bk.a, UsArgs{d_q, d_pos, B, delim});
                HIP_TRY(ctx, hipGetLastError());
                HIP_TRY(ctx, hipMemcpyAsync(hpos.data(), d_pos, hq.size() * 4, hipMemcpyDeviceToHost, st));
                HIP_TRY(ctx, bzh_stream_wait(st));
            }
            uint64_t batch_end = 0;
            if (!walk.place(ent, B, hpos.data(), out_offs, out_lens, pfirst, pc, &batch_end, &bad)) return table_mismatch();
            if (batch_end > cap) over = true; // (locating goes on: the caller learns the room needed)
            if (over) {
                pc.clear();
                pfirst.assign((size_t)B + 1, 0);
            }
            qs.pieces += pc.size();
            BackPieces bp;
            BZH_TRY(fr.pieces(pfirst.data(), pc, B, cap, bp, &qs.blocks_whole));
            BZH_TRY(back_emit(ctx, w, clock, fr.bk, d_out, true, fr.blocks, false, &bp));
            BZH_TRY(fr.crcs(ent, B));
            t0 += B;
        }
        clock.collect();
    }
    walk.finish(out_offs, out_lens);
    *out_total = (size_t)walk.run_off;
    if (over || walk.run_off > cap) {
        bzh_set_error(ctx, "decode records: the records hold %llu bytes, the buffer %zu", (unsigned long long)walk.run_off, cap);
        return BZH_E_CAP;
    }
    ds.out_bytes = walk.run_off;
    return BZH_OK;
}

// The record table of decoded bytes d_raw[0 .. n) under an index of them (idx has passed decode_index_check and sums to n).
int count_records_run(bzh_ctx *ctx, const uint8_t *d_raw, size_t n, uint8_t delim, const bzh_index_entry *idx, size_t count, uint64_t *rec_cum,
                      uint64_t *nrecords)
{
    hipStream_t st = ctx->stream;
    rec_cum[0] = 0;
    *nrecords = 0;
    if (count == 0) return BZH_OK;
    std::vector<uint64_t> offs(count);
    std::vector<uint32_t> lens(count), tfirst(count + 1);
    uint64_t tiles = 0;
    for (size_t e = 0; e < count; e++) {
        offs[e] = idx[e].out_off;
        lens[e] = idx[e].out_len;
        tfirst[e] = (uint32_t)tiles;
        tiles += ((uint64_t)idx[e].out_len + CB_TILE - 1) / CB_TILE;
        if (tiles > 0x7FFFFFFFull) {
            bzh_set_error(ctx, "count records: %zu bytes under %zu entries are beyond one launch", n, count);
            return BZH_E_ARG;
        }
    }
    tfirst[count] = (uint32_t)tiles;
    uint8_t lastb = 0;
    std::vector<uint32_t> tcount((size_t)tiles);
    if (tiles) {
        uint64_t *d_offs = nullptr;
        uint32_t *d_lens = nullptr, *d_tfirst = nullptr, *d_tcount = nullptr;
        BZH_TRY(reserve_cut(ctx, ctx->records_ws, "the record tables", grow_mib, [&](Carver &c) {
            c.put(d_offs, count), c.put(d_lens, count), c.put(d_tfirst, count + 1), c.put(d_tcount, (size_t)tiles);
        }));
        HIP_TRY(ctx, hipMemcpyAsync(d_offs, offs.data(), count * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(d_lens, lens.data(), count * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(d_tfirst, tfirst.data(), (count + 1) * 4, hipMemcpyHostToDevice, st));
        count_bytes_blocks<<<dim3((uint32_t)tiles), CB_THREADS, 0, st>>>(d_raw, d_offs, d_lens, d_tfirst, (uint32_t)count, delim, d_tcount);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(tcount.data(), d_tcount, (size_t)tiles * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(&lastb, d_raw + (n - 1), 1, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, bzh_stream_wait(st));
    }
    for (size_t e = 0; e < count; e++) {
        uint64_t d = 0;
        for (uint32_t t = tfirst[e]; t < tfirst[e + 1]; t++) d += tcount[t];
        rec_cum[e + 1] = rec_cum[e] + d;
    }
    *nrecords = rec_cum[count] + (n > 0 && lastb != delim);
    return BZH_OK;
}

// ================================================================================================================
// A range of an indexed input, window by window into a sink (bzh_search_range*, bzh_grep_index*): windows of consecutive touched
// entries through the indexed front and the back, WHOLE blocks at sink.front of the sink's staging buffer.  The sink is told the
// range -- begin(), here and only here -- and applies it; the walk knows the sink by WindowSink alone (the windows' sizes:
// bzf_window_blocks, search_plan.h; the target: bzh_search_set_room).  With a record table the walk also holds every entry's
// delimiters against it; only the range search passes one, and the text of that refusal is its own.
// ================================================================================================================
constexpr size_t SEARCH_ROOM = (size_t)128 << 20; // the default bzhip.h documents

// (idx has passed decode_index_check, pts decode_sync_check, rec_cum -- null without BZH_SEARCH_RECORDS -- bzq_table_check)
int decode_range_sink_run(bzh_ctx *ctx, const uint8_t *d_in, size_t n, uint64_t in_byte_base, const bzh_index_entry *idx, size_t count,
                          const bzh_sync_point *pts, size_t npts, const uint64_t *rec_cum, uint64_t off, uint64_t len, WindowSink &sink)
{
    size_t first, last;
    uint64_t byte_lo, byte_hi, clipped;
    index_span(idx, count, off, len, &first, &last, &byte_lo, &byte_hi, &clipped); // the wanted range, clipped to the output
    if (clipped == 0 || last <= first) return BZH_OK;
    if (sink.look_behind || sink.look_ahead) { // the decoded range: the neighbours the sink looks at lie in it (the sink keeps to the wanted one)
        const uint64_t w_off = off - std::min<uint64_t>(off, sink.look_behind), w_len = clipped + (off - w_off) + sink.look_ahead;
        uint64_t w_clipped;
        index_span(idx, count, w_off, w_len, &first, &last, &byte_lo, &byte_hi, &w_clipped);
    }
    BZH_TRY(index_covered(ctx, idx, first, last - 1, in_byte_base, n));
    DecWs w;
    BZH_TRY(dec_ws(ctx, w));
    BackCount bc{sink.delim, nullptr, nullptr, {}, {}};
    if (rec_cum) BZH_TRY(back_count_ws(ctx, bc));
    StageClock clock{ctx, {}};
    const size_t Bmax = batch_max(ctx);
    const uint64_t room = ctx->search_room ? ctx->search_room : SEARCH_ROOM;
    sink.begin(off, off + clipped, idx[first].out_off, rec_cum ? rec_cum[first] : 0);
    std::vector<uint32_t> ent;
    IndexedFront fr{ctx, w, clock, d_in, n, in_byte_base, idx, pts, npts};
    for (size_t at = first; at < last;) {
        uint64_t bytes = 0;
        const uint32_t B = (uint32_t)bzf_window_blocks(idx, at, last, room, Bmax, &bytes);
        ent.resize(B);
        for (uint32_t k = 0; k < B; k++) ent[k] = (uint32_t)(at + k);
        BZH_TRY(fr.run(ent.data(), B, rec_cum ? &bc : nullptr)); // (the sizes are the entries': checked)
        for (uint32_t k = 0; rec_cum && k < B; k++) {
            uint64_t d = 0;
            for (uint32_t t = 0; t < (fr.blocks[k].nblock + UR_TILE - 1) / UR_TILE; t++) d += bc.tcount[(size_t)k * w.T + t];
            if (d != rec_cum[at + k + 1] - rec_cum[at + k]) {
                bzh_set_error(ctx, "search range: the record table does not match entry %zu", at + k);
                return BZH_E_DATA;
            }
        }
        uint8_t *d_stage = nullptr;
        BZH_TRY(sink.room(ctx, bytes, &d_stage));
        uint64_t local = 0;
        for (uint32_t k = 0; k < B; k++) {
            BackBlock &b = fr.blocks[k];
            b.lo = 0, b.hi = (uint32_t)b.size;
            b.base = (int64_t)(sink.front + local);
            local += b.size;
        }
        BZH_TRY(back_emit(ctx, w, clock, fr.bk, d_stage, true, fr.blocks));
        BZH_TRY(fr.crcs(ent.data(), B));
        BZH_TRY(sink.window(ctx, bytes));
        at += B;
    }
    clock.collect();
    ctx->dstats.out_bytes = clipped;
    return BZH_OK;
}
