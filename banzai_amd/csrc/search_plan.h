// search_plan.h -- the windows of a search and what is carried between them (bzh_search*, search.hip / decode.hip).  Pure host
// arithmetic, no launch in it: the library compiles it, and tests/decode_host/search_host.cpp runs it against brute force per
// output byte.
//
// A WINDOW is what the staging buffer holds at one time: `bytes` decoded bytes of the output, whole blocks, at staging position
// `front`.  The last plen - 1 bytes of everything seen so far (the CARRY) lie in front of them, at [front - carry, front), so that
// a match may begin in one window and end in the next.
//   * A match that starts in the carry cannot end in it (the carry is shorter than the pattern), so it was not reported by the
//     window before, which reports only matches that end inside it: no hit is found twice, none is lost.
//   * The delimiters of the carry WERE counted by the window before: a window counts from `front` on.  A hit that starts in the
//     carry has the running count less the delimiters between it and `front`.
//   * Starts are clipped to the wanted range [lo, hi) of the output: a hit lies wholly inside it.
// The host keeps the running output offset, hit rank and delimiter count.
#ifndef BZH_SEARCH_PLAN_H
#define BZH_SEARCH_PLAN_H
#include <stddef.h>
#include <stdint.h>

constexpr uint64_t BZF_FRONT = 512; // staging position of a window's first byte (a multiple of 16, above the longest carry)

struct BzfWindow { // what the two passes over one window are given, in staging positions
    uint64_t n;          // the text is [0, n); nothing behind it is looked at
    uint64_t s_lo, s_hi; // start positions that are reported (s_lo == s_hi: none); s_hi + plen - 1 <= n
    uint64_t d_lo;       // delimiters count in [d_lo, n)
    uint64_t off_base;   // output offset of a hit at position p: off_base + p (modulo 2^64)
    uint64_t rank_base;  // hits in front of the window
    uint64_t rec_base;   // delimiters of the output in front of position d_lo
    uint64_t emit;       // of the window's hits, in order, the first `emit` are stored (at hit slots rank_base ..)
};

struct BzfWalk {
    uint32_t plen = 1;
    uint64_t front = BZF_FRONT;
    uint64_t max = 0;        // hit slots of the caller
    uint64_t lo = 0, hi = 0; // the wanted range of the output
    uint64_t out_pos = 0;    // output offset of the next window's first byte
    uint64_t carry = 0;      // bytes in front of it that are carried
    uint64_t rank = 0;       // hits so far
    uint64_t recs = 0;       // delimiters in output [0, out_pos)

    // out_start: the output offset of the first window's first byte; rec_start: the delimiters in front of it
    void begin(uint32_t plen_, uint64_t front_, uint64_t max_, uint64_t lo_, uint64_t hi_, uint64_t out_start, uint64_t rec_start)
    {
        plen = plen_, front = front_, max = max_, lo = lo_, hi = hi_;
        out_pos = out_start, recs = rec_start, carry = 0, rank = 0;
    }
    // the next window: `bytes` new bytes at `front`, `hits_known` false
    BzfWindow window(uint64_t bytes) const
    {
        BzfWindow w{};
        w.n = front + bytes;
        w.d_lo = front;
        w.off_base = out_pos - front;
        w.rank_base = rank;
        w.rec_base = recs;
        const uint64_t end = out_pos + bytes;                 // (of the output seen so far)
        const uint64_t from = out_pos - carry > lo ? out_pos - carry : lo;
        const uint64_t upto = end < hi ? end : hi;            // a reported match ends at or in front of it
        if (upto >= plen && upto - plen + 1 > from) {
            w.s_lo = front + (from - out_pos);                // (from may lie in the carry: the difference wraps and comes back)
            w.s_hi = front + (upto - plen + 1 - out_pos);
        } else {
            w.s_lo = w.s_hi = front;
        }
        return w;
    }
    // of `hits` found in the window, how many the caller's array still takes
    uint64_t emit(uint64_t hits) const
    {
        const uint64_t room = rank < max ? max - rank : 0;
        return hits < room ? hits : room;
    }
    // bytes carried behind a window of `bytes` (they are its last ones, or, of a window shorter than that, it and the old carry's tail)
    uint64_t carry_after(uint64_t bytes) const
    {
        const uint64_t have = carry + bytes;
        return have < (uint64_t)plen - 1 ? have : (uint64_t)plen - 1;
    }
    // the window is done: it held `hits` hits and `delims` delimiters in [d_lo, n)
    void advance(uint64_t bytes, uint64_t hits, uint64_t delims)
    {
        carry = carry_after(bytes);
        out_pos += bytes;
        rank += hits;
        recs += delims;
    }
};

// THE HOLD-BACK WALK of a set search (bzh_search_patset*; an automaton is a set here).  Hits are pairs (start, pattern) and ascend
// by start, then by length; with several lengths "a window reports the matches that end inside it" would break that order, so the
// grep's hold-back is used instead.  An automaton with assertions (regex_core.h: LOOK) sees one byte in front of a start
// (look_behind) and one byte behind a match (look_ahead); NO ASSERTION is the case where both are 0, and ctxb stays 0 with them.
// plen holds max_len.
//   * a window that is not the last processes the STARTS in front of its last max_len - 1 + look_ahead bytes: a match from a
//     processed start ends look_ahead bytes in front of the window's end at the latest, so the byte behind it lies in the window.
//     The bytes held back are carried, and the next window, which sees every match from there to its end, processes them;
//   * the last window processes every start; a match is bounded by *lim, the end of the text or of the wanted range;
//   * the call therefore ends with a finishing window over the carry, without new bytes, when bytes are held back;
//   * the carry keeps look_behind more bytes, in front of the first start no window has processed: CONTEXT ONLY (`ctxb` of them,
//     none while the first unprocessed start is the first byte the call has seen).  Such a byte is never a start;
//   * the delimiters of the carry were counted by the window that held it back, as above;
//   * the longest carry is max_len + 1 = 257 bytes, below BZF_FRONT;
//   * the position of output offset 0 in a window is 0 - off_base: there the context in front is the text's edge.
struct BzmSetWalk : BzfWalk {
    uint32_t look_behind = 0, look_ahead = 0;
    uint64_t ctxb = 0; // bytes of the carry in front of the first unprocessed start

    void begin_look(uint32_t look_behind_, uint32_t look_ahead_) { look_behind = look_behind_, look_ahead = look_ahead_, ctxb = 0; }
    // the first start (output offset) the windows up to this one leave unprocessed
    uint64_t next_start(uint64_t bytes, bool last) const
    {
        const uint64_t end = out_pos + bytes, keep = (uint64_t)plen - 1 + look_ahead, held = out_pos - carry + ctxb;
        return last ? end : (end - held > keep ? end - keep : held);
    }
    // the next window: `bytes` new bytes at `front`; last: nothing follows
    BzfWindow window_set(uint64_t bytes, bool last, uint64_t *lim) const
    {
        BzfWindow w{};
        w.n = front + bytes;
        w.d_lo = front;
        w.off_base = out_pos - front;
        w.rank_base = rank;
        w.rec_base = recs;
        w.s_lo = w.s_hi = front;
        *lim = w.n;
        const uint64_t end = out_pos + bytes, held = out_pos - carry + ctxb; // held: the first start no window has processed
        const uint64_t p_hi = next_start(bytes, last);
        const uint64_t from = held > lo ? held : lo;
        const uint64_t bound = end < hi ? end : hi;                         // a reported match ends at or in front of it
        const uint64_t upto = p_hi < bound ? p_hi : bound;
        if (upto > from) {
            w.s_lo = front + (from - out_pos);                              // (from may lie in the carry: the difference wraps and comes back)
            w.s_hi = front + (upto - out_pos);
            *lim = front + (bound - out_pos);
        }
        return w;
    }
    // bytes carried behind a window of `bytes` that is not the last: from look_behind bytes in front of the next start on, as far
    // as the call has seen any
    uint64_t carry_after_set(uint64_t bytes) const
    {
        const uint64_t seen = out_pos - carry, next = next_start(bytes, false);
        return out_pos + bytes - (next - seen > look_behind ? next - look_behind : seen);
    }
    // the window is done; behind the last one nothing is carried
    void advance_set(uint64_t bytes, uint64_t hits, uint64_t delims, bool last)
    {
        const uint64_t next = next_start(bytes, last), keep = last ? 0 : carry_after_set(bytes);
        ctxb = last ? 0 : next - (out_pos + bytes - keep);
        carry = keep;
        out_pos += bytes;
        rank += hits;
        recs += delims;
    }
};

// The blocks of one window of a range search: as many consecutive entries from `at` on as the staging target takes, at least one,
// at most bmax.  Returns their number, *bytes their decoded sizes' sum.
template <class E>
static inline size_t bzf_window_blocks(const E *idx, size_t at, size_t last, uint64_t room, size_t bmax, uint64_t *bytes)
{
    size_t k = 0;
    uint64_t sum = 0;
    while (at + k < last && k < bmax && (k == 0 || sum + idx[at + k].out_len <= room)) sum += idx[at + k].out_len, k++;
    *bytes = sum;
    return k;
}

#endif // BZH_SEARCH_PLAN_H
