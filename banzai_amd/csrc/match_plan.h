// match_plan.h -- the windows of bzh_match* (match.hip) and what is carried between them: the hold-back walk of a set search
// (search_plan.h: BzmSetWalk) and one word more, THE CURSOR.  Pure host arithmetic, no launch in it: the library compiles it, and
// tests/decode_host/match_host.cpp runs it against a greedy loop over the whole text.
//
// THE RULE.  For a start s that holds a match, L(s) in 1..256 is the length of the longest match there.  The selection walks a
// cursor from output offset 0: the next selected match is at the lowest s >= cursor that holds one, and the cursor becomes
// s + L(s).  It runs over the whole decoded text, not line by line.
//
// THE WINDOWS are a set search's: a window that is not the last processes the starts in front of its last max_len - 1 + look_ahead
// bytes, so every processed start sees its longest match whole; the bytes held back are carried, and the last window or the
// finishing one processes them where they lie.  A single string keeps the same walk with plen = its length (its starts end
// plen - 1 in front of the text's end, which is what the hold-back leaves).  THE CURSOR is kept in output coordinates and may lie
// beyond the window's last byte: a match selected at a processed start may end in the bytes held back.  The next window clips its
// starts to it -- a held-back start in front of the cursor is dropped, one at or behind it is selected as if no edge were there --
// so the kernels always enter a window's first tile at its first byte (match_core.h).
#ifndef BZH_MATCH_PLAN_H
#define BZH_MATCH_PLAN_H
#include "search_plan.h"

enum : uint32_t {
    MT_T_SEL = 0, // selected matches of the window
    MT_T_BYTES,   // their bytes
    MT_T_DEL,     // delimiters in [d_lo, n)
    MT_T_CURSOR,  // the position behind the last selected match (where MT_T_SEL is not 0)
    MT_T_CAND,    // starts that hold a match
    MT_T_ENTERED, // tiles entered beyond their first byte
    MT_T_OPEN,    // tiles whose map is not constant
    MT_TOTALS
};

struct MtWindow {
    BzfWindow w;       // n, the processed starts [s_lo, s_hi) clipped to the cursor, d_lo, off_base, rec_base; rank_base: the matches in front
    uint64_t lim;      // a match ends at or in front of it
    uint64_t out_base; // selected bytes in front of the window
};

struct MtWalk {
    BzmSetWalk walk;
    bool by_lim = true;  // the matcher bounds a match by lim itself (patset_core.h: BY_LIM)
    uint64_t cursor = 0; // output offset: no start in front of it is selected any more
    uint64_t sel = 0, out_bytes = 0;
    bool want_out = false, want_ent = false, over = false;
    uint64_t cap = 0, max = 0;
    uint64_t candidates = 0, entered = 0, open = 0, carry_peak = 0;

    void begin(uint32_t plen, uint32_t look_behind, uint32_t look_ahead, bool by_lim_, bool want_out_, uint64_t cap_, bool want_ent_, uint64_t max_)
    {
        walk.begin(plen, BZF_FRONT, 0, 0, ~0ull, 0, 0);
        walk.begin_look(look_behind, look_ahead);
        by_lim = by_lim_, want_out = want_out_, cap = cap_, want_ent = want_ent_, max = max_;
        cursor = sel = out_bytes = 0, over = false;
        candidates = entered = open = carry_peak = 0;
    }
    // the next window: `bytes` new bytes at `front`; last: nothing follows
    MtWindow window(uint64_t front, uint64_t bytes, bool last)
    {
        walk.front = front;
        MtWindow m{};
        m.w = walk.window_set(bytes, last, &m.lim);
        BzfWindow &w = m.w;
        if (!by_lim) { // a single string's match ends inside the text
            const uint64_t hi = m.lim >= walk.plen ? m.lim - walk.plen + 1 : 0;
            if (w.s_hi > hi) w.s_hi = hi;
        }
        const uint64_t held = walk.out_pos - walk.carry + walk.ctxb; // the first start no window has processed
        if (cursor > held) {
            const uint64_t c = front + (cursor - walk.out_pos); // (the cursor may lie in the carry: the difference wraps and comes back)
            if (c > w.s_lo) w.s_lo = c;
        }
        if (w.s_lo >= w.s_hi) w.s_lo = w.s_hi = front;
        w.rank_base = sel;
        m.out_base = out_bytes;
        return m;
    }
    bool runs(const MtWindow &m, bool records) const { return m.w.n > 0 && (m.w.s_hi > m.w.s_lo || records); }
    // of a window with these totals: are its bytes and entries written?  A room that is asked for and too small ends the writing
    // for the rest of the call; the counts go on.
    bool gather(const uint64_t *t)
    {
        if ((want_ent && sel + t[MT_T_SEL] > max) || (want_out && out_bytes + t[MT_T_BYTES] > cap)) over = true;
        return !over && (want_out || want_ent) && t[MT_T_SEL] > 0;
    }
    uint64_t carry_after(uint64_t bytes) const { return walk.carry_after_set(bytes); }
    void advance(const MtWindow &m, uint64_t bytes, const uint64_t *t, bool last)
    {
        if (t[MT_T_SEL]) cursor = m.w.off_base + t[MT_T_CURSOR];
        walk.advance_set(bytes, t[MT_T_SEL], t[MT_T_DEL], last);
        sel += t[MT_T_SEL], out_bytes += t[MT_T_BYTES];
        candidates += t[MT_T_CAND], entered += t[MT_T_ENTERED], open += t[MT_T_OPEN];
        if (walk.carry > carry_peak) carry_peak = walk.carry;
    }
    bool overflow() const { return over; }
};

#endif // BZH_MATCH_PLAN_H
