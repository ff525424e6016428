// sync_emit.hip -- the encoder writes the sync points of the stream it is writing (bzh_encode_index*).
//
// A sync point (include/bzhip.h) is the state of a DECODER's entropy stage in front of a group of 50 symbols: bit position,
// bytes of the last column written, the pending RUNA/RUNB run and the MTF list.  The decoder finds it by walking the block
// (decode_core.h, rec.point); the encoder holds all of it when a batch is packed:
//   * which byte of the last column emits symbol t = 50 * group: the tiles' output offsets (MtfTile::off after mtf_prefix) name
//     the tile, the run heads inside it and the digits of their zero runs (mtf_tile_last's rule) the head and the digit;
//   * the MTF list there: the keys at the tile's entry (tlast after mtf_prefix), raised by the last occurrences between the
//     tile's start and that head -- place = names with a larger key, the rule mtf_walk_par starts its tiles from;
//   * the bit: the block's offset, its header bits, the pack tile's offset (bt.symbits) and the code lengths of the symbols of
//     that pack tile in front of t, read as pack_tilebits reads them.
// One wavefront per point.  tlast / MtfTile live in bt.listA / bt.listB, which nothing after mtf_run writes (the Huffman stage
// keeps its scratch in bt.tagg), so the launch goes behind the batch's pack, where the host waits anyway.
#include "common.h"

constexpr uint32_t SE_SYMS = 258; // symbols of a coding table (huffman.hip: HUF_SYMS)
constexpr uint32_t SE_GROUP = 50; // symbols of a group (huffman.hip: SEG)

struct SyncEmitArgs {
    uint32_t interval;   // groups between two points, >= 1
    uint32_t MT, TL;     // MTF tiles per block stride and bytes per tile, as mtf_run laid them out for this batch
    uint32_t PT, selmax; // pack tiles per block stride, selectors per block stride (huff_prepare)
    uint32_t entry_base; // index entry of the batch's first block
    uint64_t bit_base;   // stream bit of the batch's first block
};

__device__ __forceinline__ uint32_t se_points(uint32_t m, uint32_t interval) // points of a block of m symbols
{
    return ((m + SE_GROUP - 1) / SE_GROUP - 1) / interval;
}

// FX: BZH_MODE_FIXED -- the table of a group comes from bt.fx_sel
template <bool FX>
__global__ void __launch_bounds__(64) sync_emit(Batch bt, const int32_t *tlast, const MtfTile *rt, SyncEmitArgs a, bzh_sync_point *out,
                                                uint32_t out_cap)
{
    const uint32_t b = blockIdx.y, k = blockIdx.x;
    const uint32_t lane = threadIdx.x;
    const uint32_t m = bt.m[b];
    if (k >= se_points(m, a.interval)) return;
    const uint32_t group = (k + 1) * a.interval, t = group * SE_GROUP; // t < m: the group exists
    uint32_t slot = 0; // points of the blocks before this one
    for (uint32_t bb = lane; bb < b; bb += 64) slot += se_points(bt.m[bb], a.interval);
    slot = wave_all_add(slot) + k;
    if (slot >= out_cap) return; // (the host sized the array from the same counts)

    __shared__ uint8_t names[256], inv[256];
    __shared__ int keys[256];
    __shared__ __attribute__((aligned(16))) uint8_t sb[16 + 2 * MTF_TILE + 16]; // sb[16 + i] = byte i of the tile, sb[15] the byte before it
    __shared__ int res[3];                                                        // g, pg, j
    __shared__ uint32_t pw[72];                                                   // the point
    const uint32_t n = bt.n[b];
    const uint32_t ntile = (n + a.TL - 1) / a.TL;
    const MtfTile *rb = rt + (size_t)b * a.MT;

    // ---- names of the present bytes and back (lib/mtf.rs:17-24)
    uint32_t num_names = 0;
    for (uint32_t r = 0; r < 4; r++) {
        const uint32_t c = r * 64 + lane;
        const bool present = bt.hasbyte[(size_t)b * 256 + c] != 0;
        const unsigned long long pm = __ballot(present);
        const uint32_t nm = num_names + (uint32_t)__popcll(pm & ((1ull << lane) - 1ull));
        names[c] = (uint8_t)nm;
        if (present) inv[nm] = (uint8_t)c;
        num_names += (uint32_t)__popcll(pm);
    }
    // ---- the tile that emits symbol t: the last one whose offset is not behind t (offsets ascend; a tile without a head
    // emits nothing and shares its offset with the next one)
    uint32_t tile = 0;
    for (uint32_t t0 = 0; t0 < ntile; t0 += 64) {
        const uint32_t tt = t0 + lane;
        const bool ok = tt < ntile && rb[tt].off <= t;
        tile += (uint32_t)__popcll(__ballot(ok));
    }
    tile = tile ? tile - 1 : 0; // (tile 0 has offset 0)
    const MtfTile me = rb[tile];
    const uint32_t rel = t - me.off; // symbols of the tile in front of t
    const uint32_t base_p = tile * a.TL;
    const uint32_t tile_len = min(a.TL, n - base_p);
    const uint8_t *s = bt.bwt + (size_t)b * bt.S;
    for (uint32_t i = lane * 16; i < tile_len; i += 1024) // (S is a multiple of the tile: the load stays inside the block's stride)
        *reinterpret_cast<uint4 *>(&sb[16 + i]) = *reinterpret_cast<const uint4 *>(s + base_p + i);
    if (lane == 0) sb[15] = base_p ? s[base_p - 1] : (uint8_t)0;
    const int32_t *kin = tlast + ((size_t)b * a.MT + tile) * 256;
    for (uint32_t r = 0; r < 4; r++) keys[r * 64 + lane] = kin[r * 64 + lane];
    for (uint32_t i = lane; i < 72; i += 64) pw[i] = 0;
    if (lane == 0) res[0] = -1;
    __syncthreads();

    // ---- 64 bytes at a time, lane = byte: the run heads (mtf_tile_last's rule), the symbols each one emits (the digits of the
    // zero run in front of it, then its position), and the head g whose symbols hold t; keys are raised by the bytes in front of g
    int prev = me.last;  // the last head before the 64 in hand
    uint32_t base = 0;   // symbols of the tile emitted before them
    bool found = false;
    for (uint32_t r0 = 0; r0 < tile_len && !found; r0 += 64) {
        const uint32_t idx = r0 + lane, p = base_p + idx;
        const bool valid = idx < tile_len;
        const uint32_t c = sb[16 + idx], pc = sb[15 + idx];
        // position 0 of the block follows the front of the initial list, name 0 (lib/mtf.rs:39-43)
        const bool head = valid && (p == 0 ? names[c] != 0 : c != pc);
        const unsigned long long hm = __ballot(head);
        const unsigned long long below = hm & ((1ull << lane) - 1ull);
        const int mypg = below ? (int)(base_p + r0) + 63 - __clzll((long long)below) : prev;
        const uint32_t d = head ? run_digits((uint32_t)((int)p - 1 - mypg)) : 0u;
        const uint32_t cnt = head ? d + 1u : 0u;
        const uint32_t incl = wave_incl_add_dpp(cnt);
        const bool owner = head && base + incl - cnt <= rel && rel < base + incl;
        if (owner) {
            res[0] = (int)p;
            res[1] = mypg;
            res[2] = (int)(rel - base - (incl - cnt));
        }
        __syncthreads();
        const int g = res[0];
        found = g >= 0;
        const uint32_t lim = found ? (uint32_t)g : base_p + tile_len; // keys rise by the bytes in front of g
        if (valid && p < lim && (p + 1 >= lim || sb[17 + idx] != c)) atomicMax(&keys[names[c]], (int)p);
        if (hm) prev = (int)(base_p + r0) + 63 - __clzll((long long)hm);
        base += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    }
    __syncthreads();
    // symbols behind the last head's are the trailing run and the end of block, which mtf_prefix wrote: a head at g = n
    const int g = found ? res[0] : (int)n;
    const int pg = found ? res[1] : prev;
    const uint32_t j = found ? (uint32_t)res[2] : rel - base; // digits of g's run already emitted
    const uint32_t z = (uint32_t)(g - 1 - pg), d = run_digits(z);
    uint32_t run = z, run_weight = 1u << d; // all digits out (0, 1 without a run)
    if (j < d) {
        run = 0;
        for (uint32_t q = 0; q < j; q++) run += ((((z + 1u) >> q) & 1u) + 1u) << q;
        run_weight = 1u << j;
    }
    // ---- the MTF list: place of a name = names with a larger key
    {
        uint32_t place[4] = {0, 0, 0, 0};
        int mine[4];
#pragma unroll
        for (int q = 0; q < 4; q++) mine[q] = keys[q * 64 + lane];
        for (uint32_t jn = 0; jn < num_names; jn++) {
            const int kj = keys[jn];
#pragma unroll
            for (int q = 0; q < 4; q++) place[q] += kj > mine[q] ? 1u : 0u;
        }
        uint8_t *mtf = reinterpret_cast<uint8_t *>(pw + 8);
#pragma unroll
        for (int q = 0; q < 4; q++)
            if ((uint32_t)q * 64 + lane < num_names) mtf[place[q]] = inv[q * 64 + lane];
    }
    // ---- the bit: code lengths of the symbols of t's pack tile in front of t
    uint32_t bits = 0;
    {
        const uint16_t *sy = bt.syms + (size_t)b * (bt.S + 64);
        const uint32_t nsyms = bt.nsyms[b];
        const uint32_t *codes = FX ? bt.fx_codes + (size_t)b * FX_TABLES * SE_SYMS : bt.codes + (size_t)b * SE_SYMS;
        const uint32_t ntab = FX ? bt.ntab[b] : 1u;
        const uint8_t *sel = bt.fx_sel + (size_t)b * a.selmax;
        for (uint32_t q = t / PACK_TILE * PACK_TILE + lane; q < t; q += 64) {
            const uint32_t sym = sy[q];
            const uint32_t tab = FX ? sel[q / SE_GROUP] : 0u;
            if (sym < nsyms && tab < ntab) bits += codes[tab * SE_SYMS + sym] >> 24;
        }
        bits = wave_all_add(bits);
    }
    if (lane == 0) {
        const uint32_t *hb = bt.hdrbits + (size_t)b * 4;
        const uint64_t pos = a.bit_base + bt.bitoff[b] + hb[0] + hb[1] + hb[2] + bt.symbits[(size_t)b * a.PT + t / PACK_TILE] + bits;
        pw[0] = (uint32_t)pos;
        pw[1] = (uint32_t)(pos >> 32);
        pw[2] = a.entry_base + b;
        pw[3] = group;
        pw[4] = (uint32_t)(pg + 1); // bytes written: up to the last head, the pending run not included
        pw[5] = run;
        pw[6] = run_weight;
    }
    __syncthreads();
    uint32_t *o = reinterpret_cast<uint32_t *>(out + slot);
    o[lane] = pw[lane];
    if (lane < 8) o[64 + lane] = pw[64 + lane];
}

// Blocks 0..B-1 of the batch in the arena are plan blocks k0.., packed from stream bit `bit_base` on, and the stream has been
// waited for: their entries and sync points are appended to ix.
int sync_emit_batch(bzh_ctx *ctx, uint32_t B, size_t k0, uint64_t bit_base, EncIndex &ix)
{
    Batch &bt = ctx->bt;
    if (B == 0) return BZH_OK;
    hipStream_t st = ctx->stream;
    std::vector<uint32_t> hm(B);
    std::vector<uint64_t> off(B + 1);
    HIP_TRY(ctx, hipMemcpyAsync(hm.data(), bt.m, (size_t)B * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(off.data(), bt.bitoff, ((size_t)B + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, bzh_stream_wait(st));
    const uint32_t entry_base = (uint32_t)ix.entries.size();
    uint64_t out_off = ix.entries.empty() ? 0 : ix.entries.back().out_off + ix.entries.back().out_len;
    size_t npts = 0;
    uint32_t maxper = 0;
    for (uint32_t b = 0; b < B; b++) {
        const bzh_block &pb = ctx->plan_blocks[k0 + b];
        bzh_index_entry e;
        e.bit_pos = bit_base + off[b];
        e.end_bit = bit_base + off[b + 1];
        e.out_off = out_off;
        e.out_len = (uint32_t)pb.in_len;
        e.crc = pb.crc;
        e.stream = 0;
        e.level = (uint32_t)ctx->level;
        out_off += pb.in_len;
        ix.entries.push_back(e);
        if (ix.interval) {
            const uint32_t per = ((hm[b] + SE_GROUP - 1) / SE_GROUP - 1) / ix.interval;
            npts += per;
            maxper = std::max(maxper, per);
        }
    }
    if (npts == 0) return BZH_OK;
    if (npts > 0xFFFFFFFFull / sizeof(bzh_sync_point)) {
        bzh_set_error(ctx, "%zu sync points in one batch", npts);
        return BZH_E_NOMEM;
    }
    BZH_TRY(ctx->sync_ws.reserve(ctx, npts * sizeof(bzh_sync_point), "the sync points of a batch"));
    SyncEmitArgs a;
    a.interval = ix.interval;
    a.TL = mtf_tile_bytes(B);
    a.MT = (bt.S + a.TL - 1) / a.TL;
    a.PT = (bt.S + 64 + PACK_TILE - 1) / PACK_TILE; // as huff_prepare
    a.selmax = (bt.S + 64 + 49) / 50 + 2;
    a.entry_base = entry_base;
    a.bit_base = bit_base;
    const int32_t *tlast = mtf_tlast(bt); // (as mtf_run left them)
    const MtfTile *rt = mtf_tiles(bt);
    bzh_sync_point *d_pts = ctx->sync_ws.as<bzh_sync_point>();
    if (ctx->mode == BZH_MODE_FIXED)
        sync_emit<true><<<dim3(maxper, B), 64, 0, st>>>(bt, tlast, rt, a, d_pts, (uint32_t)npts);
    else
        sync_emit<false><<<dim3(maxper, B), 64, 0, st>>>(bt, tlast, rt, a, d_pts, (uint32_t)npts);
    HIP_TRY(ctx, hipGetLastError());
    const size_t at = ix.pts.size();
    ix.pts.resize(at + npts);
    HIP_TRY(ctx, hipMemcpyAsync(ix.pts.data() + at, d_pts, npts * sizeof(bzh_sync_point), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, bzh_stream_wait(st));
    return BZH_OK;
}
