// grep_ctx_plan.h -- the windows of a grep with context records and what is carried between them (bzh_grep_set_context), beside
// grep_plan.h's BzgWalk.  Pure host arithmetic, no launch in it: the library compiles it, and
// tests/decode_host/grep_ctx_host.cpp runs it against brute force with grep_ctx_core.h as the device.
//
// THE CARRY is *pending records, open record, held bytes*.  The last two are BzgWalk's.  The PENDING RECORDS are closed records
// that no window could judge: they lie beyond the reach (`after`) of the last primary, and a primary of the next window may lie
// within `before` of them.  With g records closed since the last primary (all closed records, if there was none) they are the
// last min(before, g - after) of them, a suffix of the closed records.  They are not primary, and that is final.  The next
// window sees their delimiters, for bytes, entries and numbering, looks for no match in them and does not count them again.
//   * Besides BzgWalk's three words, g rides along, saturated at after + before + 1, and the number of pending records.
//   * The call ends with a finishing window over the carry if bytes are held back or records are pending -- a primary tail
//     selects the pending records in front of it -- and then the open tail, once: primary, context (within `after` of a primary),
//     or neither.
//   * Rooms: as BzgWalk's.
#ifndef BZH_GREP_CTX_PLAN_H
#define BZH_GREP_CTX_PLAN_H
#include "grep_ctx_core.h"
#include "grep_plan.h"

struct BzcWalk {
    uint32_t plen = 1, invert = 0, before = 0, after = 0;
    bool want_out = false, want_ent = false;
    uint64_t cap = 0, max = 0;
    uint64_t out_pos = 0;    // output offset of the next window's first new byte
    uint64_t carry = 0;      // bytes in front of it that are carried,
    uint64_t pend_bytes = 0; // ... of which the first are the pending records,
    uint64_t held = 0;       // ... and the last `held` are not processed yet
    uint64_t npend = 0;      // the pending records
    uint64_t back = 0;       // records closed since the last primary, the pending ones included (saturated; none so far: saturated)
    uint32_t open_hit = 0;
    uint64_t recs = 0;       // records closed so far, the pending ones included
    uint64_t sel = 0, out_bytes = 0;
    uint64_t matched = 0, context = 0, groups = 0;
    bool fits = true;
    uint64_t carry_peak = 0, pending_peak = 0;

    uint64_t sat_a() const { return (uint64_t)after + before + 1; }
    void begin(uint32_t plen_, bool invert_, uint32_t before_, uint32_t after_, bool want_out_, uint64_t cap_, bool want_ent_, uint64_t max_)
    {
        *this = BzcWalk{};
        plen = plen_, invert = invert_ ? 1u : 0u, before = before_, after = after_;
        want_out = want_out_, cap = cap_, want_ent = want_ent_, max = max_;
        back = sat_a();
    }
    // the next window: `bytes` new bytes at `front` (front >= carry); last: nothing follows
    BzcWindow window(uint64_t front, uint64_t bytes, bool last) const
    {
        BzgWalk plain;
        plain.plen = plen, plain.invert = invert, plain.out_pos = out_pos, plain.carry = carry - pend_bytes, plain.held = held;
        plain.open_hit = open_hit, plain.recs = recs - npend, plain.sel = sel, plain.out_bytes = out_bytes;
        BzcWindow w{};
        w.w = plain.window(front, bytes, last);
        w.q_lo = front - carry;
        w.back_in = back - npend;
        w.sat_a = sat_a(), w.sat_b = (uint64_t)before + 1;
        w.before = before, w.after = after;
        w.last = last ? 1u : 0u;
        return w;
    }
    // whether the window has anything to do; if not, its totals are those of totals_idle
    bool runs(const BzcWindow &w) const { return w.w.n > 0 && (w.w.p_hi > w.w.p_lo || npend > 0); }
    void totals_idle(const BzcWindow &w, uint64_t *totals) const
    {
        for (uint32_t j = 0; j < BZC_TOTALS; j++) totals[j] = 0;
        totals[BZG_T_DEL] = npend, totals[BZG_T_TAIL_START] = w.w.t_lo, totals[BZG_T_TAIL_HIT] = open_hit;
        totals[BZC_T_BACK] = back, totals[BZC_T_PEND_N] = npend, totals[BZC_T_PEND_START] = w.q_lo;
    }
    bool gather(const uint64_t *totals)
    {
        if (want_out && out_bytes + totals[BZG_T_BYTES] > cap) fits = false;
        if (want_ent && sel + totals[BZG_T_SEL] > max) fits = false;
        return fits && (want_out || want_ent) && totals[BZG_T_SEL] > 0;
    }
    // the window is done; the carry of the next is buffer[totals[PEND_START], w.n)
    void advance(const BzcWindow &w, uint64_t bytes, const uint64_t *totals)
    {
        recs += totals[BZG_T_DEL] - npend;
        sel += totals[BZG_T_SEL];
        out_bytes += totals[BZG_T_BYTES];
        matched += totals[BZC_T_PRIM], context += totals[BZC_T_CTX], groups += totals[BZC_T_GROUPS];
        open_hit = (uint32_t)totals[BZG_T_TAIL_HIT];
        back = totals[BZC_T_BACK];
        npend = totals[BZC_T_PEND_N];
        carry = w.w.n - totals[BZC_T_PEND_START];
        pend_bytes = totals[BZG_T_TAIL_START] - totals[BZC_T_PEND_START];
        held = w.w.n - w.w.p_hi;
        out_pos += bytes;
        if (carry > carry_peak) carry_peak = carry;
        if (npend > pending_peak) pending_peak = npend;
    }
    // behind the finishing window (held == 0, nothing pending): the open tail is the carry; a record if it is not empty
    bool tail_primary() const { return carry > 0 && (open_hit != 0) != (invert != 0); }
    bool tail_selected() const { return carry > 0 && (tail_primary() || back + 1 <= after); }
    uint64_t nrecords() const { return recs + (carry > 0); }
    void tail_rooms(bool *copy, bool *entry)
    {
        *copy = *entry = false;
        if (!tail_selected()) return;
        if (want_out && out_bytes + carry > cap) fits = false;
        if (want_ent && sel + 1 > max) fits = false;
        *copy = fits && want_out, *entry = fits && want_ent;
    }
    BzgEntry tail_entry() const { return BzgEntry{recs, out_pos - carry, carry | (tail_primary() ? 0 : BZC_LEN_CONTEXT), out_bytes}; }
    void tail_done()
    {
        if (!tail_selected()) return;
        // a group of its own unless the record in front of it is selected: within `after` of a primary, or in front of a primary tail
        if (tail_primary() && !(recs > 0 && (before > 0 || back <= after))) groups++;
        if (tail_primary()) matched++;
        else context++;
        sel++, out_bytes += carry;
    }
    bool overflow() const { return !fits; }
};

#endif // BZH_GREP_CTX_PLAN_H
