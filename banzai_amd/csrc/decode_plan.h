// decode_plan.h -- the host arithmetic between the decoder's kernels: where a tile's bytes go inside its block, which bytes of a
// block a range wants, and which segments a batch's sync points cut its blocks into.  No HIP types: decode.hip's host side
// calls these, and tests/decode_host/plan_host.cpp compiles the same text with g++ -fsanitize=address,undefined and holds each
// against brute force.  An off-by-one here is an out-of-bounds store on the device, and this is where it can be found first.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

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
