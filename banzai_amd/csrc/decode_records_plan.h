// decode_records_plan.h -- the host arithmetic of reads by record number (bzh_record_spans, bzh_decode_records*): the check of
// an untrusted record table, the clipping of record ranges, which entries they touch, and -- batch by batch -- which delimiters
// have to be located on the device (the queries of unrle_select) and, once they are, which bytes of which block go where.  No
// HIP types: decode.hip's host side calls these, and tests/decode_host/records_host.cpp compiles the same text with
// g++ -fsanitize=address,undefined and holds each against brute force per output byte.
//
// The terms are include/bzhip.h's: D delimiters at p_1 < .. < p_D, record r = bytes [s_r, e_r), s_0 = 0, s_r = p_r + 1,
// e_r = s_(r+1), e_D = total.  A range {first, len} of records is the bytes [s_first, s_(first+len)), with s_k = total for k > D.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

#include "decode_plan.h" // PieceRef, bzp_window

struct BzqQuery { // one launch of unrle_select: the k-th (1-based) delimiter of tile `tile` of the block in batch slot `slot`
    uint32_t slot, tile, k, pad;
};
constexpr uint32_t BZQ_NONE = 0xFFFFFFFFu; // unrle_select's answer to a query nothing satisfies

// What makes the table ill formed against the index (null: nothing); *bad = the entry.  rec_cum holds count + 1 words.
template <class E>
static inline const char *bzq_table_check(const E *idx, size_t count, const uint64_t *rec_cum, size_t *bad)
{
    *bad = 0;
    if (rec_cum[0] != 0) return "rec_cum[0] is not 0";
    for (size_t e = 0; e < count; e++) {
        *bad = e;
        if (rec_cum[e + 1] < rec_cum[e]) return "the counts descend";
        if (rec_cum[e + 1] - rec_cum[e] > idx[e].out_len) return "more delimiters than the entry has bytes";
    }
    return nullptr;
}

// The records [*a, *b) of {off, len} clipped to the D + 1 records there are; off + len saturates.
static inline void bzq_clip(uint64_t D, uint64_t off, uint64_t len, uint64_t *a, uint64_t *b)
{
    const uint64_t nrec = D + 1; // (D <= the indexed total < 2^64 - 1)
    *a = off < nrec ? off : nrec;
    *b = len < nrec - *a ? *a + len : nrec;
}

// The first range that begins in front of the end of the one before it, after clipping (nranges: none does).  R: bzh_range.
template <class R>
static inline size_t bzq_ranges_check(const R *ranges, size_t nranges, uint64_t D)
{
    uint64_t end = 0;
    for (size_t r = 0; r < nranges; r++) {
        uint64_t a, b;
        bzq_clip(D, ranges[r].off, ranges[r].len, &a, &b);
        if (a < end) return r;
        end = b;
    }
    return nranges;
}

// The entry whose bytes hold delimiter k, 1 <= k <= rec_cum[count]: the first e with rec_cum[e + 1] >= k.  The search stays
// inside the table whatever it holds and answers below `count` (count >= 1).
static inline size_t bzq_entry_of(const uint64_t *rec_cum, size_t count, uint64_t k)
{
    size_t lo = 0, hi = count - 1;
    while (lo < hi) {
        const size_t mid = lo + (hi - lo) / 2;
        if (rec_cum[mid + 1] < k)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// The entries [*first, *last] a clipped, non-empty range [a, b) of records touches (count >= 1): from the block that holds
// delimiter a -- entry 0 for a == 0 -- to the block that holds delimiter b, or the last entry when b > D.  The block of a
// boundary delimiter is touched also when the delimiter is its last byte and it gives the range no byte: only the decode says so.
static inline void bzq_entry_span(const uint64_t *rec_cum, size_t count, uint64_t a, uint64_t b, size_t *first, size_t *last)
{
    const uint64_t D = rec_cum[count];
    *first = a == 0 ? 0 : bzq_entry_of(rec_cum, count, a);
    *last = b <= D ? bzq_entry_of(rec_cum, count, b) : count - 1;
    if (*last < *first) *last = *first; // (only a table that does not ascend gets here)
}

// The entries the ranges touch, ascending and unique, and the hull of their compressed bytes (0 and 0 with nothing touched).
// The ranges need not ascend here.  An empty range (after clipping) touches nothing.
template <class E, class R>
static inline void bzq_spans(const E *idx, size_t count, const uint64_t *rec_cum, const R *ranges, size_t nranges,
                             std::vector<uint32_t> &touched, uint64_t *byte_lo, uint64_t *byte_hi)
{
    std::vector<uint64_t> runs; // first << 32 | last + 1
    for (size_t r = 0; count && r < nranges; r++) {
        uint64_t a, b;
        bzq_clip(rec_cum[count], ranges[r].off, ranges[r].len, &a, &b);
        if (a == b) continue;
        size_t first, last;
        bzq_entry_span(rec_cum, count, a, b, &first, &last);
        runs.push_back((uint64_t)first << 32 | (uint64_t)(last + 1));
    }
    std::sort(runs.begin(), runs.end());
    touched.clear();
    uint32_t next = 0;
    for (uint64_t run : runs)
        for (uint32_t e = std::max(next, (uint32_t)(run >> 32)); e < (uint32_t)run; e++) {
            touched.push_back(e);
            next = e + 1;
        }
    *byte_lo = touched.empty() ? 0 : idx[touched.front()].bit_pos / 8;
    *byte_hi = touched.empty() ? 0 : (idx[touched.back()].end_bit + 7) / 8;
}

// The walk of one bzh_decode_records call over its touched entries, in ascending batches.  The ranges ascend and do not overlap
// (bzq_ranges_check), so when a batch is placed every earlier range has ended in it or before: the running output offset is
// known, and no block is needed twice.  Per batch: queries() once the tile counts are back, then place() once the positions are.
template <class E, class R>
struct BzqWalk {
    const E *idx = nullptr;
    size_t count = 0;
    const uint64_t *rec_cum = nullptr;
    uint64_t D = 0, total = 0;
    struct Rg {
        uint64_t a, b;       // clipped records
        int64_t ja, jb;      // its boundaries in `bounds` (-1: the start is byte 0 / the end is the total)
        size_t first, last;  // entries
    };
    std::vector<Rg> rg; // every range, the empty ones too (a == b)
    struct Bound {
        uint64_t k;    // the delimiter's number, 1..D
        size_t entry;  // that holds it
        uint64_t byte; // the output byte behind it, once located
        bool located;
    };
    std::vector<Bound> bounds; // ascending, unique
    size_t jnext = 0;          // the first boundary not yet asked for
    size_t rnext = 0;          // the first range not yet ended
    uint64_t run_off = 0;      // bytes of the ranges before it
    bool started = false;      // range rnext has its offset
    std::vector<size_t> qbound; // the boundary of every query of the batch

    // `touched` as bzq_spans lists it.  False: the ranges do not ascend, *bad names the first that does not.
    bool start(const E *idx_, size_t count_, const uint64_t *rec_cum_, const R *ranges, size_t nranges, size_t *bad)
    {
        idx = idx_, count = count_, rec_cum = rec_cum_;
        D = count ? rec_cum[count] : 0;
        total = count ? idx[count - 1].out_off + idx[count - 1].out_len : 0;
        rg.clear(), bounds.clear();
        jnext = rnext = 0, run_off = 0, started = false;
        *bad = bzq_ranges_check(ranges, nranges, D);
        if (*bad != nranges) return false;
        auto bound = [&](uint64_t k) {
            if (bounds.empty() || bounds.back().k != k) bounds.push_back({k, bzq_entry_of(rec_cum, count, k), 0, false});
            return (int64_t)bounds.size() - 1;
        };
        for (size_t r = 0; r < nranges; r++) {
            Rg g = {0, 0, -1, -1, 0, 0};
            bzq_clip(D, ranges[r].off, ranges[r].len, &g.a, &g.b);
            if (count == 0) g.b = g.a; // (no entries: every record is empty)
            if (g.a != g.b) {
                bzq_entry_span(rec_cum, count, g.a, g.b, &g.first, &g.last);
                if (g.a > 0) g.ja = bound(g.a);
                if (g.b <= D) g.jb = bound(g.b);
            }
            rg.push_back(g);
        }
        return true;
    }

    // The queries of the batch whose blocks are the entries ent[0 .. B) (a slice of the touched list), block k in slot k with
    // ntiles[k] tiles whose delimiter counts are tcount[k * stride ..].  False: the tiles of *bad do not sum to the table's count.
    bool queries(const uint32_t *ent, uint32_t B, const uint32_t *tcount, uint32_t stride, const uint32_t *ntiles, std::vector<BzqQuery> &q,
                 size_t *bad)
    {
        q.clear(), qbound.clear();
        for (uint32_t k = 0; k < B; k++) {
            uint64_t sum = 0;
            for (uint32_t t = 0; t < ntiles[k]; t++) sum += tcount[(size_t)k * stride + t];
            if (sum != rec_cum[ent[k] + 1] - rec_cum[ent[k]]) {
                *bad = ent[k];
                return false;
            }
        }
        for (; jnext < bounds.size() && bounds[jnext].entry <= ent[B - 1]; jnext++) {
            const Bound &bd = bounds[jnext];
            const uint32_t k = (uint32_t)(std::lower_bound(ent, ent + B, (uint32_t)bd.entry) - ent);
            if (k >= B || ent[k] != bd.entry) continue; // (an entry in front of the batch: only a caller that skips batches)
            uint64_t j = bd.k - rec_cum[bd.entry]; // 1 .. the block's count: the tiles sum to it
            uint32_t t = 0;
            while (t + 1 < ntiles[k] && j > tcount[(size_t)k * stride + t]) j -= tcount[(size_t)k * stride + t++];
            q.push_back({k, t, (uint32_t)j, 0});
            qbound.push_back(jnext);
        }
        return true;
    }

    // pos[i] = unrle_select's answer to query i: the delimiter's position in its block's output.  Then the pieces of the batch's
    // blocks: block k has pc[pfirst[k] .. pfirst[k + 1]), in range order (as bzp_block_pieces lays them out), and the ranges that
    // end in this batch get their out_offs / out_lens (size_t[nranges], every range's by the last batch).  *batch_end = the
    // highest output byte a piece of this batch reaches.  False: an answer that is no byte of its block; *bad names the entry.
    bool place(const uint32_t *ent, uint32_t B, const uint32_t *pos, size_t *out_offs, size_t *out_lens, std::vector<size_t> &pfirst,
               std::vector<PieceRef> &pc, uint64_t *batch_end, size_t *bad)
    {
        for (size_t i = 0; i < qbound.size(); i++) {
            Bound &bd = bounds[qbound[i]];
            if (pos[i] == BZQ_NONE || pos[i] >= idx[bd.entry].out_len) {
                *bad = bd.entry;
                return false;
            }
            bd.byte = idx[bd.entry].out_off + pos[i] + 1;
            bd.located = true;
        }
        struct Want {
            uint32_t k;
            PieceRef p;
        };
        std::vector<Want> wants;
        *batch_end = 0;
        const size_t e_lo = ent[0], e_hi = ent[B - 1];
        for (; rnext < rg.size(); rnext++, started = false) {
            const Rg &g = rg[rnext];
            if (g.a == g.b) {
                out_offs[rnext] = (size_t)run_off;
                out_lens[rnext] = 0;
                continue;
            }
            if (g.first > e_hi || (g.ja >= 0 && !bounds[g.ja].located)) break; // it begins in a later batch
            const uint64_t S = g.ja >= 0 ? bounds[g.ja].byte : 0;
            const bool ended = g.jb >= 0 ? bounds[g.jb].located : g.last <= e_hi;
            const uint64_t En = g.jb >= 0 ? (ended ? bounds[g.jb].byte : total) : total;
            if (!started) out_offs[rnext] = (size_t)run_off;
            started = true;
            const size_t f = std::max(g.first, e_lo), l = std::min(g.last, e_hi);
            for (size_t e = f; e <= l && f <= l; e++) {
                const uint32_t k = (uint32_t)(std::lower_bound(ent, ent + B, (uint32_t)e) - ent);
                if (k >= B || ent[k] != e) continue;
                PieceRef p;
                bzp_window(idx[e].out_off, idx[e].out_len, S, En, &p.lo, &p.hi);
                if (p.lo >= p.hi) continue;
                p.base = run_off + (idx[e].out_off + p.lo - S);
                *batch_end = std::max(*batch_end, p.base + (p.hi - p.lo));
                wants.push_back({k, p});
            }
            if (!ended) break;
            out_lens[rnext] = (size_t)(En - S);
            run_off += En - S;
        }
        pfirst.assign((size_t)B + 1, 0);
        for (const Want &w : wants) pfirst[w.k + 1]++;
        for (uint32_t k = 0; k < B; k++) pfirst[k + 1] += pfirst[k];
        pc.resize(wants.size());
        std::vector<size_t> cursor(pfirst.begin(), pfirst.end() - 1);
        for (const Want &w : wants) pc[cursor[w.k]++] = w.p;
        return true;
    }

    // Behind the last batch: the empty ranges behind the last one that touched anything.  run_off is the sum of all lengths.
    void finish(size_t *out_offs, size_t *out_lens)
    {
        for (; rnext < rg.size(); rnext++) {
            out_offs[rnext] = (size_t)run_off;
            out_lens[rnext] = 0;
        }
    }
};
