// decode.hip -- the bzip2 DECODER (bzh_decode*, include/bzhip.h).  The reference has none (README.md:9); the format is the
// one it writes (lib/lib.rs:18-70, lib/huffman.rs:464-572) and libbz2 reads.
//
//   scan     : every occurrence of the block and the footer magic, at any bit alignment     (decode_scan_kernel)
//   entropy  : one wavefront per candidate: header, tables, symbols -> last column           (decode_block_kernel, decode_core.h)
//   chain    : the host walks from block end to block start; candidates inside a payload drop out
//   unbwt    : the inverse transform of the batch                                            (unbwt_run, bwt.hip)
//   unrle    : inverse RLE1 -- roles by a scan of state maps, sizes, then the expansion      (unrle_maps / unrle_walk)
//   crc      : block CRCs over the output ranges (rle1.hip), folded per stream on the host
#include <algorithm>
#include <type_traits>
#include <vector>

#include "common.h"
#include "decode_core.h"

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

// ---- inverse RLE1 ----------------------------------------------------------------------------------------------
// A tile = 4096 bytes of a block, 16 a thread.  unrle_maps: the tile's state map.  unrle_walk<false>: the tile's entry state
// (the maps of the tiles before it, composed) and its output bytes; <true>: the expansion, at offsets the host has summed.
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
    __device__ __forceinline__ uint32_t at(int k) const { return (w[k >> 2] >> (8 * (k & 3))) & 255u; }
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

__device__ __forceinline__ uint32_t ur_thread_map(const UrBytes &u)
{
    uint32_t st[5] = {0, 1, 2, 3, 4};
    uint32_t prev = u.prev;
#pragma unroll
    for (int k = 0; k < (int)UR_ITEMS; k++) {
        if ((uint32_t)k < u.cnt) {
            const uint32_t c = u.at(k);
            const bool eq = c == prev;
#pragma unroll
            for (int s = 0; s < 5; s++) st[s] = bzd_rl_step(st[s], eq);
            prev = c;
        }
    }
    return st[0] | st[1] << 3 | st[2] << 6 | st[3] << 9 | st[4] << 12;
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

__global__ void __launch_bounds__(UR_THREADS) unrle_maps(UrArgs a)
{
    __shared__ uint32_t lds[4];
    const uint32_t b = a.slots[blockIdx.y], t = blockIdx.x, n = a.n[b];
    const UrBytes u = ur_load(a.x + (size_t)b * a.S, n, t * UR_TILE + threadIdx.x * UR_ITEMS);
    uint32_t total;
    (void)ur_scan(ur_thread_map(u), lds, &total);
    if (threadIdx.x == 0) a.tmap[(size_t)b * a.T + t] = total;
}

template <bool EXPAND>
__global__ void __launch_bounds__(UR_THREADS) unrle_walk(UrArgs a)
{
    __shared__ uint32_t lds[8];
    __shared__ uint8_t stage[EXPAND ? UR_STAGE : 4];
    const uint32_t b = a.slots[blockIdx.y], t = blockIdx.x, n = a.n[b];
    const size_t ti = (size_t)b * a.T + t;
    uint32_t entry, total;
    if (EXPAND) {
        entry = a.tstate[ti];
    } else { // the tiles before this one, a thread each (T <= UR_THREADS: the host checks)
        const uint32_t m = threadIdx.x < t ? a.tmap[(size_t)b * a.T + threadIdx.x] : BZD_RL_ID;
        (void)ur_scan(m, lds, &total);
        entry = bzd_rl_apply(total, 0);
        if (threadIdx.x == 0) a.tstate[ti] = entry;
    }
    const uint32_t i0 = t * UR_TILE + threadIdx.x * UR_ITEMS;
    const UrBytes u = ur_load(a.x + (size_t)b * a.S, n, i0);
    const uint32_t ex = ur_scan(ur_thread_map(u), lds, &total);
    uint32_t s = bzd_rl_apply(ex, entry);
    uint32_t outn = 0, prev = u.prev;
#pragma unroll
    for (int k = 0; k < (int)UR_ITEMS; k++) {
        if ((uint32_t)k < u.cnt) {
            const uint32_t c = u.at(k);
            outn += s == 4 ? c : 1u;
            s = bzd_rl_step(s, c == prev);
            prev = c;
        }
    }
    uint32_t tile_total;
    const uint32_t o0 = block_excl_add(outn, lds, &tile_total);
    if (!EXPAND) {
        if (threadIdx.x == 0) a.tout[ti] = tile_total;
        if (u.cnt && i0 + u.cnt == n) a.endstate[b] = s;
        return;
    }
    if (tile_total == 0) return;
    const bool staged = tile_total <= UR_STAGE;
    uint8_t *g = a.out + a.obase[blockIdx.y] + a.toff[ti];
    uint32_t o = o0;
    s = bzd_rl_apply(ex, entry);
    prev = u.prev;
    // (every offset is checked against the tile's total, which is the sum the host laid the output out by)
#pragma unroll
    for (int k = 0; k < (int)UR_ITEMS; k++) {
        if ((uint32_t)k < u.cnt) {
            const uint32_t c = u.at(k);
            if (s == 4) {
                for (uint32_t q = 0; q < c; q++, o++)
                    if (o < tile_total) {
                        if (staged)
                            stage[o] = (uint8_t)prev;
                        else
                            g[o] = (uint8_t)prev;
                    }
            } else {
                if (o < tile_total) {
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
    // the staged tile goes out in aligned words, its ragged edges byte by byte
    const uint32_t head = min(tile_total, (uint32_t)((0 - (uintptr_t)g) & 3u));
    const uint32_t words = (tile_total - head) / 4, tail0 = head + words * 4;
    if (threadIdx.x < head) g[threadIdx.x] = stage[threadIdx.x];
    for (uint32_t i = threadIdx.x; i < words; i += UR_THREADS) {
        const uint8_t *sp = stage + head + 4 * i;
        *reinterpret_cast<uint32_t *>(g + head + 4 * i) = (uint32_t)sp[0] | (uint32_t)sp[1] << 8 | (uint32_t)sp[2] << 16 | (uint32_t)sp[3] << 24;
    }
    if (tail0 + threadIdx.x < tile_total) g[tail0 + threadIdx.x] = stage[tail0 + threadIdx.x];
}

// ---- host side ---------------------------------------------------------------------------------------------------
struct DecWs { // carved from ctx->dec_ws (allocated on the first decode: an encode-only user pays nothing)
    uint64_t *cand;    // [B]
    BzdResult *res;    // [B]
    uint32_t *tmap, *tout, *tstate, *toff; // [B][T]
    uint32_t *endstate, *slots, *crcacc;   // [B]
    uint64_t *obase;   // [B]
    BlockDesc *desc;   // [B]
    uint32_t *scancnt; // [1]
    uint32_t B, T;
};

static int dec_ws(bzh_ctx *ctx, DecWs &w)
{
    const size_t B = ctx->max_batch, T = ctx->S / UR_TILE;
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    const size_t need = up(B * 8) + up(B * sizeof(BzdResult)) + 4 * up(B * T * 4) + 3 * up(B * 4) + up(B * 8) + up(B * sizeof(BlockDesc)) + 256;
    if (!ctx->dec_ws || ctx->dec_ws_size < need) {
        if (ctx->dec_ws) hipFree(ctx->dec_ws);
        ctx->dec_ws = nullptr;
        ctx->dec_ws_size = 0;
        if (hipMalloc((void **)&ctx->dec_ws, need) != hipSuccess) {
            bzh_set_error(ctx, "hipMalloc(%zu) for the decode tables failed", need);
            return BZH_E_NOMEM;
        }
        ctx->dec_ws_size = need;
    }
    uint8_t *p = ctx->dec_ws;
    auto take = [&](auto *&dst, size_t bytes) {
        dst = reinterpret_cast<std::remove_reference_t<decltype(dst)>>(p);
        p += up(bytes);
    };
    take(w.cand, B * 8);
    take(w.res, B * sizeof(BzdResult));
    take(w.tmap, B * T * 4);
    take(w.tout, B * T * 4);
    take(w.tstate, B * T * 4);
    take(w.toff, B * T * 4);
    take(w.endstate, B * 4);
    take(w.slots, B * 4);
    take(w.crcacc, B * 4);
    take(w.obase, B * 8);
    take(w.desc, B * sizeof(BlockDesc));
    take(w.scancnt, 4);
    w.B = (uint32_t)B;
    w.T = (uint32_t)T;
    return BZH_OK;
}

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
    for (int attempt = 0; attempt < 2; attempt++) {
        if (!ctx->dec_list || ctx->dec_list_cap == 0) {
            const size_t cap = 65536;
            if (hipMalloc((void **)&ctx->dec_list, cap * 8) != hipSuccess) return BZH_E_NOMEM;
            ctx->dec_list_cap = cap;
        }
        HIP_TRY(ctx, hipMemsetAsync(w.scancnt, 0, 4, st));
        decode_scan_kernel<<<dim3((uint32_t)wgs), SCAN_THREADS, 0, st>>>(d_in, n, ctx->dec_list, (uint32_t)ctx->dec_list_cap, w.scancnt);
        HIP_TRY(ctx, hipGetLastError());
        uint32_t cnt = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&cnt, w.scancnt, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, bzh_stream_wait(st));
        if (cnt <= ctx->dec_list_cap) {
            cands.resize(cnt);
            if (cnt) HIP_TRY(ctx, hipMemcpy(cands.data(), ctx->dec_list, (size_t)cnt * 8, hipMemcpyDeviceToHost));
            std::sort(cands.begin(), cands.end());
            return BZH_OK;
        }
        hipFree(ctx->dec_list); // more hits than the list holds: once more with one that does
        ctx->dec_list = nullptr;
        ctx->dec_list_cap = 0;
        const size_t cap = (size_t)cnt + 1024;
        if (hipMalloc((void **)&ctx->dec_list, cap * 8) != hipSuccess) return BZH_E_NOMEM;
        ctx->dec_list_cap = cap;
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
};
} // namespace

// The chain walk and the back of the decoder.  cands: decode_scan_run's list.  The arena holds min(cands, max_batch) blocks.
int decode_chain_run(bzh_ctx *ctx, const uint8_t *d_in, size_t n, uint8_t *d_out, size_t cap, size_t *out_len, size_t *consumed,
                     const std::vector<uint64_t> &cands)
{
    hipStream_t st = ctx->stream;
    Batch &bt = ctx->bt;
    bzh_decode_stats &ds = ctx->dstats;
    DecWs w;
    BZH_TRY(dec_ws(ctx, w));
    if (w.T > UR_THREADS) {
        bzh_set_error(ctx, "decode: %u tiles a block exceed the walk kernel's %u threads (internal error)", w.T, UR_THREADS);
        return BZH_E_STATE;
    }
    std::vector<StageSpan> spans;
    auto mark = [&]() -> hipEvent_t {
        if (!ctx->profiling) return nullptr;
        hipEvent_t e = bzh_event(ctx);
        hipEventRecord(e, st);
        return e;
    };
    auto span = [&](int stage, hipEvent_t a) {
        if (a) spans.push_back({stage, a, mark()});
    };
    auto collect = [&]() {
        double *dst[5] = {&ds.ms_scan, &ds.ms_entropy, &ds.ms_unbwt, &ds.ms_unrle, &ds.ms_crc};
        for (auto &s : spans) {
            float t = 0;
            if (hipEventElapsedTime(&t, s.a, s.b) == hipSuccess) *dst[s.stage] += t;
        }
        spans.clear();
    };
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
    const size_t nc = cands.size();
    const uint64_t nbits = (uint64_t)n * 8;
    uint64_t pos = 32, total_out = 0;
    uint32_t stream_crc = 0;
    size_t ci = 0;
    bool finished = false, over = false;
    std::vector<BzdResult> res;
    std::vector<ChainItem> items;
    std::vector<uint32_t> slots, hout, hoff, hend;
    std::vector<uint64_t> hbase, hsize;
    std::vector<BlockDesc> hdesc;
    while (!finished) {
        while (ci < nc && (cands[ci] >> 1) < pos) {
            ds.candidates_off_chain++;
            ci++;
        }
        if (ci == nc || (cands[ci] >> 1) != pos) return data_error(pos + 48 > nbits ? BZD_K_TRUNC : BZD_K_MAGIC, pos, "neither a block nor a footer");
        const uint32_t B = (uint32_t)std::min<size_t>(std::min<size_t>(ctx->max_batch, ctx->arena_blocks), nc - ci);
        hipEvent_t e0 = mark();
        HIP_TRY(ctx, hipMemcpyAsync(w.cand, cands.data() + ci, (size_t)B * 8, hipMemcpyHostToDevice, st));
        decode_block_kernel<<<dim3(B), 64, 0, st>>>(d_in, n, w.cand, bt, w.res, 100000u * (uint32_t)ctx->level);
        HIP_TRY(ctx, hipGetLastError());
        span(1, e0);
        res.resize(B);
        HIP_TRY(ctx, hipMemcpyAsync(res.data(), w.res, (size_t)B * sizeof(BzdResult), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, bzh_stream_wait(st));
        // the chain through this batch
        items.clear();
        slots.clear();
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
                items.push_back({false, k, r.crc, stream, block, cpos});
                slots.push_back(k);
                block++;
                ds.blocks++;
                pos = r.end_bit;
                continue;
            }
            items.push_back({true, k, r.crc, stream, block, cpos});
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
        const uint32_t K = (uint32_t)slots.size();
        if (K) {
            const uint32_t Bu = slots.back() + 1;
            uint32_t nmax_all = 1, nmax = 1;
            for (uint32_t s = 0; s < Bu; s++)
                if (!(cands[ci - k + s] & 1ull) && res[s].kind == BZD_OK) nmax_all = std::max(nmax_all, res[s].nblock);
            for (uint32_t s : slots) nmax = std::max(nmax, res[s].nblock);
            hipEvent_t e1 = mark();
            BZH_TRY(unbwt_run(ctx, Bu, nmax_all));
            span(2, e1);
            hipEvent_t e2 = mark();
            UrArgs a{};
            a.x = bt.mtfpos;
            a.n = bt.n;
            a.slots = w.slots;
            a.S = bt.S;
            a.T = w.T;
            a.tmap = w.tmap;
            a.tout = w.tout;
            a.tstate = w.tstate;
            a.endstate = w.endstate;
            a.toff = w.toff;
            a.obase = w.obase;
            a.out = d_out;
            const uint32_t Tn = (nmax + UR_TILE - 1) / UR_TILE;
            HIP_TRY(ctx, hipMemcpyAsync(w.slots, slots.data(), (size_t)K * 4, hipMemcpyHostToDevice, st));
            unrle_maps<<<dim3(Tn, K), UR_THREADS, 0, st>>>(a);
            unrle_walk<false><<<dim3(Tn, K), UR_THREADS, 0, st>>>(a);
            HIP_TRY(ctx, hipGetLastError());
            hout.resize((size_t)Bu * w.T);
            hend.resize(Bu);
            HIP_TRY(ctx, hipMemcpyAsync(hout.data(), w.tout, hout.size() * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(ctx, hipMemcpyAsync(hend.data(), w.endstate, (size_t)Bu * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(ctx, bzh_stream_wait(st));
            hoff.assign((size_t)Bu * w.T, 0);
            hbase.resize(K);
            hsize.resize(K);
            uint64_t maxsize = 0;
            for (uint32_t q = 0; q < K; q++) {
                const uint32_t s = slots[q], tn = (res[s].nblock + UR_TILE - 1) / UR_TILE;
                uint64_t sz = 0;
                for (uint32_t t = 0; t < tn; t++) {
                    hoff[(size_t)s * w.T + t] = (uint32_t)sz;
                    sz += hout[(size_t)s * w.T + t];
                }
                if (hend[s] == 4) { // libbz2 refuses the block; the state machine says where
                    for (const ChainItem &it : items)
                        if (!it.footer && it.slot == s) {
                            stream = it.stream;
                            block = it.block;
                            return data_error(BZD_K_FORMAT, it.bitpos, "the block ends in four equal bytes without a count");
                        }
                }
                hbase[q] = total_out;
                hsize[q] = sz;
                total_out += sz;
                maxsize = std::max(maxsize, sz);
            }
            if (total_out > cap) over = true; // (sizing goes on: the caller learns the total)
            if (!over) {
                HIP_TRY(ctx, hipMemcpyAsync(w.toff, hoff.data(), hoff.size() * 4, hipMemcpyHostToDevice, st));
                HIP_TRY(ctx, hipMemcpyAsync(w.obase, hbase.data(), (size_t)K * 8, hipMemcpyHostToDevice, st));
                unrle_walk<true><<<dim3(Tn, K), UR_THREADS, 0, st>>>(a);
                HIP_TRY(ctx, hipGetLastError());
                span(3, e2);
                hipEvent_t e3 = mark();
                hdesc.resize(K);
                for (uint32_t q = 0; q < K; q++) hdesc[q] = BlockDesc{hbase[q], hsize[q], 0, 0};
                HIP_TRY(ctx, hipMemcpyAsync(w.desc, hdesc.data(), (size_t)K * sizeof(BlockDesc), hipMemcpyHostToDevice, st));
                BZH_TRY(crc_blocks_device(ctx, d_out, w.desc, w.crcacc, K, maxsize));
                HIP_TRY(ctx, hipMemcpyAsync(hdesc.data(), w.desc, (size_t)K * sizeof(BlockDesc), hipMemcpyDeviceToHost, st));
                span(4, e3);
                HIP_TRY(ctx, bzh_stream_wait(st));
            } else {
                span(3, e2);
            }
        }
        // CRCs in chain order: every block's against its header, every stream's fold against its footer
        uint32_t q = 0;
        const size_t stream_at = stream, block_at = block; // (errors below name the item they are about)
        for (const ChainItem &it : items) {
            stream = it.stream;
            block = it.block;
            if (!it.footer) {
                if (!over && hdesc[q].crc != it.crc) return data_error(BZD_K_BLOCK_CRC, it.bitpos);
                stream_crc = ((stream_crc << 1) | (stream_crc >> 31)) ^ it.crc;
                q++;
            } else {
                if (stream_crc != it.crc) return data_error(BZD_K_STREAM_CRC, it.bitpos);
                stream_crc = 0;
            }
        }
        stream = stream_at;
        block = block_at;
        if (finished) break;
    }
    collect();
    ds.candidates_off_chain += nc - ci; // (magics in foreign bytes behind the last stream)
    ds.out_bytes = total_out;
    *out_len = (size_t)total_out;
    if (over) {
        bzh_set_error(ctx, "decode: the output needs %llu bytes, the buffer holds %zu", (unsigned long long)total_out, cap);
        return BZH_E_CAP;
    }
    return BZH_OK;
}
