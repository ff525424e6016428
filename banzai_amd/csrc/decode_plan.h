// decode_plan.h -- the host arithmetic between the decoder's kernels: where a tile's bytes go inside its block, which bytes of a
// block a range wants, and which segments a batch's sync points cut its blocks into.  No HIP types: decode.hip's host side
// calls these, and tests/decode_host/plan_host.cpp compiles the same text with g++ -fsanitize=address,undefined and holds each
// against brute force.  An off-by-one here is an out-of-bounds store on the device, and this is where it can be found first.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
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

// The segments of the B blocks of a batch, the entries idx[ent[0 .. B)] (ascending, not necessarily adjacent), between those of
// the sync points pts[0 .. npts) that belong to them (ascending by entry; E: bzh_index_entry, P: bzh_sync_point).  A block with c
// points has c + 1 consecutive segments, header -> first point -> .. -> end of block.  seg0[k] = the first segment of block k,
// seg0[B] = their number.  The batch's points are gathered: pmap[j] = the point of pts that lies at j of the gathered array, which
// from / to count in (adjacent entries: pmap[j] = pmap[0] + j).
template <class E, class P>
static inline void bzp_segments(const E *idx, const uint32_t *ent, uint32_t B, const P *pts, size_t npts, std::vector<SegDesc> &segs,
                                std::vector<uint32_t> &seg0, std::vector<size_t> &pmap)
{
    segs.clear();
    pmap.clear();
    seg0.assign((size_t)B + 1, 0);
    for (uint32_t k = 0; k < B; k++) {
        seg0[k] = (uint32_t)segs.size();
        const uint32_t bmax = 100000u * idx[ent[k]].level;
        size_t lo = 0, hi = npts; // the first point of entry ent[k] or behind
        while (lo < hi) {
            const size_t mid = lo + (hi - lo) / 2;
            if (pts[mid].entry < ent[k])
                lo = mid + 1;
            else
                hi = mid;
        }
        int32_t prev = -1;
        for (size_t q = lo; q < npts && pts[q].entry == ent[k]; q++) {
            segs.push_back({k, prev, (int32_t)pmap.size(), bmax});
            prev = (int32_t)pmap.size();
            pmap.push_back(q);
        }
        segs.push_back({k, prev, -1, bmax});
    }
    seg0[B] = (uint32_t)segs.size();
}

// ---- many ranges in one call (bzh_decode_ranges*, bzh_index_spans) ---------------------------------------------------------
// The bytes of [off, off + len) inside an output of `total` bytes; off + len saturates.
static inline uint64_t bzp_clip_len(uint64_t total, uint64_t off, uint64_t len)
{
    return off < total ? (len < total - off ? len : total - off) : 0;
}

// The entries [*first, *last) that hold output bytes [off, off + clipped), clipped > 0 and inside the indexed total (E:
// bzh_index_entry).  Two binary searches that stay inside idx[0 .. count) whatever the entries hold.
template <class E>
static inline void bzp_entry_span(const E *idx, size_t count, uint64_t off, uint64_t clipped, size_t *first, size_t *last)
{
    size_t lo = 0, hi = count; // the first entry that ends behind `off`
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (idx[mid].out_off + idx[mid].out_len <= off)
            lo = mid + 1;
        else
            hi = mid;
    }
    *first = lo;
    const uint64_t end = off + clipped; // the first entry that starts at or behind the end
    hi = count;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (idx[mid].out_off < end)
            lo = mid + 1;
        else
            hi = mid;
    }
    *last = lo;
}

// Where the ranges' bytes go and which entries they touch (R: bzh_range).  out_lens[r] = the range clipped to the indexed total,
// out_offs[r] = the running sum (either may be null); touched = the union of the ranges' entries, ascending and unique;
// [*byte_lo, *byte_hi) = the bytes of the indexed input from the first touched entry's bit_pos / 8 to the last one's
// ceil(end_bit / 8), 0 and 0 with nothing touched.  Returns the sum of the clipped lengths.
template <class E, class R>
static inline uint64_t bzp_spans(const E *idx, size_t count, const R *ranges, size_t nranges, size_t *out_offs, size_t *out_lens,
                                 std::vector<uint32_t> &touched, uint64_t *byte_lo, uint64_t *byte_hi)
{
    const uint64_t total = count ? idx[count - 1].out_off + idx[count - 1].out_len : 0;
    std::vector<uint64_t> runs; // first << 32 | last, one a range that touches anything
    uint64_t sum = 0;
    for (size_t r = 0; r < nranges; r++) {
        const uint64_t c = bzp_clip_len(total, ranges[r].off, ranges[r].len);
        if (out_offs) out_offs[r] = (size_t)sum;
        if (out_lens) out_lens[r] = (size_t)c;
        sum += c;
        if (c == 0) continue;
        size_t first, last;
        bzp_entry_span(idx, count, ranges[r].off, c, &first, &last);
        if (first < last) runs.push_back((uint64_t)first << 32 | (uint64_t)last);
    }
    std::sort(runs.begin(), runs.end());
    touched.clear();
    uint32_t next = 0; // entries below it are listed
    for (uint64_t run : runs)
        for (uint32_t e = std::max(next, (uint32_t)(run >> 32)); e < (uint32_t)run; e++) {
            touched.push_back(e);
            next = e + 1;
        }
    *byte_lo = touched.empty() ? 0 : idx[touched.front()].bit_pos / 8;
    *byte_hi = touched.empty() ? 0 : (idx[touched.back()].end_bit + 7) / 8;
    return sum;
}

// A piece: bytes [lo, hi) of a block's own output, wanted at out[base .. base + hi - lo).
struct PieceRef {
    uint32_t lo, hi;
    uint64_t base;
};

// The pieces of every touched block, a piece being what one range wants of one block: block touched[j] has pieces
// pc[pfirst[j] .. pfirst[j + 1]), in the order of their ranges; prange names each piece's range.  out_offs: bzp_spans'.
template <class E, class R>
static inline void bzp_block_pieces(const E *idx, size_t count, const R *ranges, size_t nranges, const size_t *out_offs,
                                    const std::vector<uint32_t> &touched, std::vector<size_t> &pfirst, std::vector<PieceRef> &pc,
                                    std::vector<uint32_t> &prange)
{
    const uint64_t total = count ? idx[count - 1].out_off + idx[count - 1].out_len : 0;
    pfirst.assign(touched.size() + 1, 0);
    std::vector<size_t> cursor;
    for (int pass = 0; pass < 2; pass++) {
        for (size_t r = 0; r < nranges; r++) {
            const uint64_t off = ranges[r].off, c = bzp_clip_len(total, off, ranges[r].len);
            if (c == 0) continue;
            size_t first, last;
            bzp_entry_span(idx, count, off, c, &first, &last);
            if (first >= last) continue;
            // (every entry of the range is listed, and the list ascends without gaps inside a range)
            const size_t j0 = (size_t)(std::lower_bound(touched.begin(), touched.end(), (uint32_t)first) - touched.begin());
            for (size_t e = first; e < last; e++) {
                const size_t j = j0 + (e - first);
                if (pass == 0) {
                    pfirst[j + 1]++;
                    continue;
                }
                PieceRef p;
                bzp_window(idx[e].out_off, idx[e].out_len, off, off + c, &p.lo, &p.hi);
                p.base = (uint64_t)out_offs[r] + (idx[e].out_off + p.lo - off);
                pc[cursor[j]] = p;
                prange[cursor[j]++] = (uint32_t)r;
            }
        }
        if (pass == 0) {
            for (size_t j = 0; j < touched.size(); j++) pfirst[j + 1] += pfirst[j];
            pc.resize(pfirst.back());
            prange.resize(pfirst.back());
            cursor.assign(pfirst.begin(), pfirst.end() - 1);
        }
    }
}

// Which pieces meet which tile, for the K blocks of a batch that are emitted piece by piece.  Block k has the pieces
// pc[pf[k] .. pf[k + 1]) and ntiles[k] tiles, tile t putting out tout[k][t] bytes at toff[k][t] of the block (rows of `stride`
// words at tout + rows[k] * stride: the host image of the device tables).  refs[tile_first[k * Tn + t] .. tile_first[k * Tn + t
// + 1]) = the pieces that meet tile t of block k, each cut to the tile: [lo, hi) inside [toff, toff + tout), base moved along.
// A tile without output meets none.  False: more references than 32 bits count.
static inline bool bzp_pieces(const uint32_t *rows, const uint32_t *ntiles, uint32_t K, const uint32_t *tout, const uint32_t *toff,
                              uint32_t stride, uint32_t Tn, const size_t *pf, const PieceRef *pc, std::vector<uint32_t> &tile_first,
                              std::vector<PieceRef> &refs)
{
    tile_first.assign((size_t)K * Tn + 1, 0);
    std::vector<uint32_t> cursor;
    for (int pass = 0; pass < 2; pass++) {
        for (uint32_t k = 0; k < K; k++) {
            const uint32_t *o = tout + (size_t)rows[k] * stride, *f = toff + (size_t)rows[k] * stride;
            const uint32_t tn = std::min(ntiles[k], Tn);
            for (size_t q = pf[k]; q < pf[k + 1]; q++) {
                const PieceRef &p = pc[q];
                if (p.lo >= p.hi || tn == 0) continue;
                // the last tile that starts at or in front of lo; from there on while tiles start in front of hi
                uint32_t t = (uint32_t)(std::upper_bound(f, f + tn, p.lo) - f);
                t = t ? t - 1 : 0;
                for (; t < tn && f[t] < p.hi; t++) {
                    const uint32_t a = std::max(p.lo, f[t]), b = std::min(p.hi, f[t] + o[t]);
                    if (a >= b) continue;
                    const size_t cell = (size_t)k * Tn + t;
                    if (pass == 0) {
                        if (++tile_first[cell + 1] == 0) return false;
                        continue;
                    }
                    refs[cursor[cell]++] = PieceRef{a, b, p.base + (a - p.lo)};
                }
            }
        }
        if (pass == 0) {
            uint64_t sum = 0;
            for (size_t c = 1; c < tile_first.size(); c++) {
                sum += tile_first[c];
                if (sum > 0xFFFFFFFFull) return false;
                tile_first[c] = (uint32_t)sum;
            }
            refs.resize((size_t)sum);
            cursor.assign(tile_first.begin(), tile_first.end() - 1);
        }
    }
    return true;
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
