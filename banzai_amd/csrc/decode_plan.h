// decode_plan.h -- the host arithmetic between the decoder's kernels: where a tile's bytes go inside its block, which bytes of a
// block a range wants, and which segments a batch's sync points cut its blocks into.  No HIP types: decode.hip's host side
// calls these, and tests/decode_host/plan_host.cpp compiles the same text with g++ -fsanitize=address,undefined and holds each
// against brute force.  An off-by-one here is an out-of-bounds store on the device, and this is where it can be found first.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

#include "batch.h"       // BlockDesc, the carver
#include "decode_core.h" // BzdResult

struct SegDesc {
    uint32_t slot;      // of its block in the batch
    int32_t from, to;   // points of the batch it runs between; -1: the header's state / the end of the block
    uint32_t block_max; // bytes a block of its entry's level may hold
};

// toff[t] = bytes the tiles before tile t of a block put out, for the (nblock + tile - 1) / tile tiles that hold its nblock
// bytes (tout[t]: what tile t puts out); the block's decoded size.  Tiles behind the block's last are not touched.
static inline uint64_t bzp_tile_sums(const uint32_t *tout, uint32_t *toff, uint32_t nblock, uint32_t tile)
{
    const uint32_t tn = nblock / tile + (nblock % tile != 0);
    uint64_t sz = 0;
    for (uint32_t t = 0; t < tn; t++) {
        toff[t] = (uint32_t)sz;
        sz += tout[t];
    }
    return sz;
}

// The bytes [*lo, *hi) of an entry's own output (out_len bytes at out_off of the whole) that the range [off, end) wants:
// 0 <= *lo <= *hi <= out_len, empty where the two do not meet.  True: the window is the whole entry.
static inline bool bzp_window(uint64_t out_off, uint32_t out_len, uint64_t off, uint64_t end, uint32_t *lo, uint32_t *hi)
{
    const uint64_t l = off <= out_off ? 0 : off - out_off < out_len ? off - out_off : out_len;
    const uint64_t h = end <= out_off ? 0 : end - out_off < out_len ? end - out_off : out_len;
    *lo = (uint32_t)l;
    *hi = (uint32_t)(h < l ? l : h);
    return *lo == 0 && *hi == out_len;
}

// The segments of the B blocks of a batch, entries idx[e0 .. e0 + B), between the sync points pts[p0 .. p1) of those entries
// (ascending by entry; E: bzh_index_entry, P: bzh_sync_point).  A block with c points has c + 1 consecutive segments, header ->
// first point -> .. -> end of block; from / to count from p0.  seg0[k] = the first segment of block k, seg0[B] = their number.
template <class E, class P>
static inline void bzp_segments(const E *idx, size_t e0, uint32_t B, const P *pts, size_t p0, size_t p1, std::vector<SegDesc> &segs,
                                std::vector<uint32_t> &seg0)
{
    segs.clear();
    seg0.assign((size_t)B + 1, 0);
    size_t q = p0;
    for (uint32_t k = 0; k < B; k++) {
        seg0[k] = (uint32_t)segs.size();
        const uint32_t bmax = 100000u * idx[e0 + k].level;
        int32_t prev = -1;
        for (; q < p1 && pts[q].entry == e0 + k; q++) {
            segs.push_back({k, prev, (int32_t)(q - p0), bmax});
            prev = (int32_t)(q - p0);
        }
        segs.push_back({k, prev, -1, bmax});
    }
    seg0[B] = (uint32_t)segs.size();
}

// ---- the decoder's per-batch tables (decode.hip) ---------------------------------------------------------------------------
struct DecWs { // carved from ctx->dec_ws by dec_layout (allocated on the first decode: an encode-only user pays nothing)
    uint64_t *cand;    // [B]
    BzdResult *res;    // [B]
    uint32_t *tmap, *tout, *tstate, *toff; // [B][T]
    uint32_t *endstate, *slots, *crcacc;   // [B]
    uint64_t *obase;   // [B]
    BlockDesc *desc;   // [B]
    uint32_t *scancnt; // [1]
    // [B] the blocks of a batch that are not expanded whole (back_emit): cut by a range's edge, or not written at all.  wslots /
    // wbase / wacc / wcrc are twins of slots / obase / crcacc / desc[].crc because a range's batch has whole and cut blocks in flight
    // together: both walks and both CRC passes are queued before the one wait.
    uint32_t *wslots, *wlo, *whi, *bsize, *wacc, *wcrc;
    int64_t *wbase;    // [B]
    uint32_t *magic;   // [B] range_magic_kernel's verdicts
    uint32_t *small;   // [B] bzh_decode_many: the batch slots whose blocks the LDS inverse BWT takes
    uint32_t B, T;
};

// Lays the tables of batches of B blocks of T inverse-RLE1 tiles out at `base` (nullptr: only measures); the bytes they take.
static inline size_t dec_layout(DecWs &w, void *base, uint32_t B, uint32_t T, std::vector<CarveSpan> *log = nullptr)
{
    Carver c(base);
    c.log = log;
    const size_t BT = (size_t)B * T;
    c.put(w.cand, B);
    c.put(w.res, B);
    c.put(w.tmap, BT);
    c.put(w.tout, BT);
    c.put(w.tstate, BT);
    c.put(w.toff, BT);
    c.put(w.endstate, B);
    c.put(w.slots, B);
    c.put(w.crcacc, B);
    c.put(w.obase, B);
    c.put(w.desc, B);
    c.put(w.scancnt, 1);
    c.put(w.wslots, B);
    c.put(w.wlo, B);
    c.put(w.whi, B);
    c.put(w.bsize, B);
    c.put(w.wacc, B);
    c.put(w.wcrc, B);
    c.put(w.magic, B);
    c.put(w.wbase, B);
    c.put(w.small, B);
    w.B = B;
    w.T = T;
    return c.bytes();
}
