// grep_plan.h -- the windows of a grep and what is carried between them (bzh_grep*, grep.hip / decode.hip).  Pure host arithmetic,
// no launch in it: the library compiles it, and tests/decode_host/grep_host.cpp runs it against brute force with grep_core.h as
// the device.
//
// A WINDOW is what the staging buffer holds at one time: `bytes` new decoded bytes, whole blocks, at staging position `front`,
// and in front of them the CARRY: every byte behind the last delimiter a window has processed.  That is the whole open record --
// an input without a delimiter is carried whole -- and behind it the last plen - 1 bytes seen (`held`), which no window has
// processed yet: a match that starts there may end in the next window, and a pattern may hold the delimiter, so a record that ends
// there is judged by the next window, which sees the match to its end.  The text of a window therefore begins at a record start.
//   * Three words ride along: open_hit (a match already started in the processed part of the carry), the records closed so far,
//     and the output offset of the next new byte.
//   * A window emits exactly the records whose delimiter it processes; matches and delimiters are processed over the same
//     positions, so a match belongs to the record of its first byte whichever window sees it.
//   * The call ends with a window without new bytes over the carry, if bytes are held back, and then the open tail, once.
//   * Rooms: a window is gathered only while the totals so far fit every room that is asked for; after the first that does not,
//     nothing more is gathered and the call goes on counting.
#ifndef BZH_GREP_PLAN_H
#define BZH_GREP_PLAN_H
#include "grep_core.h"

struct BzgWalk {
    uint32_t plen = 1, invert = 0;
    bool want_out = false, want_ent = false; // rooms that are asked for
    uint64_t cap = 0, max = 0;
    uint64_t out_pos = 0;   // output offset of the next window's first new byte
    uint64_t carry = 0;     // bytes in front of it that are carried,
    uint64_t held = 0;      // ... of which the last `held` are not processed yet
    uint32_t open_hit = 0;
    uint64_t recs = 0;      // records closed so far
    uint64_t sel = 0;       // selected records so far,
    uint64_t out_bytes = 0; // ... and their bytes
    bool fits = true;       // the totals so far fit the rooms asked for
    uint64_t carry_peak = 0;

    void begin(uint32_t plen_, bool invert_, bool want_out_, uint64_t cap_, bool want_ent_, uint64_t max_)
    {
        *this = BzgWalk{};
        plen = plen_, invert = invert_ ? 1u : 0u, want_out = want_out_, cap = cap_, want_ent = want_ent_, max = max_;
    }
    // the next window: `bytes` new bytes at `front` (front >= carry); last: nothing follows, every position is processed
    BzgWindow window(uint64_t front, uint64_t bytes, bool last) const
    {
        BzgWindow w{};
        w.n = front + bytes;
        w.t_lo = front - carry;
        w.p_lo = front - held;
        const uint64_t keep = (uint64_t)plen - 1;
        w.p_hi = last ? w.n : (w.n >= keep && w.n - keep > w.p_lo ? w.n - keep : w.p_lo);
        const uint64_t ends = w.n + 1 >= plen ? w.n + 1 - plen : 0; // starts in front of it end inside the text
        w.s_hi = ends < w.p_hi ? (ends > w.p_lo ? ends : w.p_lo) : w.p_hi;
        w.off_base = out_pos - front;
        w.rec_base = recs;
        w.out_base = out_bytes;
        w.sel_base = sel;
        w.open_hit = open_hit;
        w.invert = invert;
        return w;
    }
    // the window's totals are known: is it gathered?  (also: from now on nothing is, if not)
    bool gather(const uint64_t *totals)
    {
        if (want_out && out_bytes + totals[BZG_T_BYTES] > cap) fits = false;
        if (want_ent && sel + totals[BZG_T_SEL] > max) fits = false;
        return fits && (want_out || want_ent) && totals[BZG_T_SEL] > 0;
    }
    // the window is done; the carry of the next is buffer[totals[TAIL_START], w.n)
    void advance(const BzgWindow &w, uint64_t bytes, const uint64_t *totals)
    {
        recs += totals[BZG_T_DEL];
        sel += totals[BZG_T_SEL];
        out_bytes += totals[BZG_T_BYTES];
        open_hit = (uint32_t)totals[BZG_T_TAIL_HIT];
        carry = w.n - totals[BZG_T_TAIL_START];
        held = w.n - w.p_hi;
        out_pos += bytes;
        if (carry > carry_peak) carry_peak = carry;
    }
    // behind the last window (held == 0): the open tail is the carry; a record if it is not empty
    bool tail_selected() const { return carry > 0 && (open_hit != 0) != (invert != 0); }
    uint64_t nrecords() const { return recs + (carry > 0); }
    // the tail is emitted: whether its bytes / its entry fit (and are asked for)
    void tail_rooms(bool *copy, bool *entry)
    {
        *copy = *entry = false;
        if (!tail_selected()) return;
        if (want_out && out_bytes + carry > cap) fits = false;
        if (want_ent && sel + 1 > max) fits = false;
        *copy = fits && want_out, *entry = fits && want_ent;
    }
    BzgEntry tail_entry() const { return BzgEntry{recs, out_pos - carry, carry, out_bytes}; }
    void tail_done()
    {
        if (tail_selected()) sel++, out_bytes += carry;
    }
    bool overflow() const { return !fits; }
};

// bytes in front of the decoders' BZF_FRONT that a staging buffer needs for a carry
static inline uint64_t bzg_front_extra(uint64_t carry, uint64_t front)
{
    const uint64_t a = (carry + 15) & ~(uint64_t)15;
    return a > front ? a - front : 0;
}

#endif // BZH_GREP_PLAN_H
