// grep_many_core.h -- MANY TEXTS IN ONE BUFFER with walls between them (bzh_grep_many*, grep_many.hip): what grep_core.h's phases
// need to know to treat every text as bzh_grep treats it alone.  Plain C++ without a launch in it: the kernels compile it for the
// device, tests/decode_host/grep_many_host.cpp for the host, where it runs thread by thread and tile by tile against a naive
// split-and-find of every text.  The tables are built on the host by grep_many_plan.h.
//
// A SEGMENT is one text: bytes [lo, hi) of the buffer.  Segments ascend and do not overlap; an empty one owns no tile.
// A VIRTUAL TILE is a pair (segment, aligned 4,096-byte tile of the buffer that it meets); the table holds them in segment order.
// A tile that several segments meet stands there once per segment: an input shorter than a tile still costs a tile's work.
//
// THE RULE.  For every segment the answer is bzh_grep's for that text alone.  The window of a virtual tile is its segment's
// (t_lo = p_lo = lo, p_hi = n = hi, nothing carried in, nothing held back); the matcher's bounds are rebound to it, so a match
// ends inside the segment and an assertion sees its two ends as the text's edges, whatever byte of a neighbour lies beside them.
// The last byte of a segment closes a record even where it is no delimiter: a delimiter bit for position hi - 1 (bzgm_close).
// That is the open tail of a single grep, which the host emits there once a call and cannot emit once an input.
//
// THE SCAN is grep_core.h's with BzgManyTexts as its rows: the hit state and the open record start anew at a segment's first
// virtual tile, no selection reaches back behind its last one, selected bytes and selected records run through the whole call.
// The delimiter count runs through the call as well; a segment's own count, in front of a tile or in all, is the difference to
// what stands in front of its first virtual tile (bzgm_base, bzgm_totals).
#ifndef BZH_GREP_MANY_CORE_H
#define BZH_GREP_MANY_CORE_H
#include "grep_core.h"
#include "regex_core.h"

struct BzgmSeg { // a row of the segment table
    uint64_t lo, hi;  // the text, in buffer coordinates
    uint32_t first;   // its first virtual tile,
    uint32_t rows;    // ... and how many it owns (0: an empty text)
};
struct BzgmRow { // a row of the virtual tile table
    uint32_t seg, tile;
};
enum : uint32_t { BZGM_T_RECORDS = 0, BZGM_T_SEL = 1, BZGM_T_BYTES = 2, BZGM_TOTALS = 3 }; // a segment's totals row

// the window of a segment: the whole text in one window, offsets and record numbers count from its start
BZF_FN BzgWindow bzgm_window(const BzgmSeg &s, uint32_t plen, uint32_t invert)
{
    BzgWindow w{};
    w.n = s.hi, w.t_lo = w.p_lo = s.lo, w.p_hi = s.hi;
    const uint64_t ends = s.hi + 1 >= plen ? s.hi + 1 - plen : 0; // (BzgWalk::window, last = true)
    w.s_hi = ends < w.p_hi ? (ends > w.p_lo ? ends : w.p_lo) : w.p_hi;
    w.off_base = 0 - s.lo;
    w.invert = invert;
    return w;
}

// the by-value matcher rebound to the text [lo, hi): lim = n = hi, edge_lo = lo, the edge context in front of it
BZF_FN void bzgm_rebind(BzfOne &, uint64_t, uint64_t) {} // (a single pattern's starts are bounded by the window's s_hi)
BZF_FN void bzgm_rebind(BzmMatcher &m, uint64_t, uint64_t hi) { m.m.lim = hi; }
template <bool LDS_ROWS>
BZF_FN void bzgm_rebind(BzrMatcher<LDS_ROWS, false> &m, uint64_t, uint64_t hi) { m.a.m.lim = hi; }
template <bool LDS_ROWS>
BZF_FN void bzgm_rebind(BzrMatcher<LDS_ROWS, true> &m, uint64_t lo, uint64_t hi)
{
    m.a.m.lim = hi;
    m.l.n = hi, m.l.edge_lo = lo, m.l.ctx_lo = BZR_LOOK_EDGE;
}

// the text's last byte closes a record: the delimiter bit of position p_hi - 1 in the thread at p0 (the window is not empty)
BZF_FN void bzgm_close(BzgThread &t, const BzgWindow &w, uint64_t p0)
{
    const uint64_t last = w.p_hi - 1;
    if (last >= p0 && last - p0 < BZF_ITEMS) t.dm |= 1u << (uint32_t)(last - p0);
}

// the rows of the scan (grep_core.h: BzgOneText)
struct BzgManyTexts {
    const BzgmRow *row;
    const BzgmSeg *seg;
    BZG_MEM uint32_t tile_no(uint32_t v) const { return row[v].tile; }
    BZG_MEM bool enters(uint32_t v, uint64_t *start) const
    {
        const BzgmSeg &s = seg[row[v].seg];
        if (s.first != v) return false;
        *start = s.lo;
        return true;
    }
    BZG_MEM bool leaves(uint32_t v) const
    {
        const BzgmSeg &s = seg[row[v].seg];
        return s.first + s.rows - 1 == v;
    }
    BZG_MEM const BzgWindow &window(uint32_t v, const BzgWindow &w, BzgWindow &cut) const
    {
        const BzgmSeg &s = seg[row[v].seg];
        cut = w;
        cut.t_lo = s.lo, cut.p_hi = s.hi;
        return cut;
    }
};

// what lies in front of virtual tile v within its text: the delimiters counted from the segment's first virtual tile
BZF_FN BzgBase bzgm_base(const BzgBase *base, uint32_t v, const BzgmSeg &s)
{
    BzgBase b = base[v];
    b.del -= base[s.first].del;
    return b;
}

// behind the scan: the totals row of segment k -- its records, its selected records and their bytes.  base: in front of every
// virtual tile; totals: the call's (BZG_T_*), what stands behind the last one
BZF_FN void bzgm_totals(const BzgmSeg *seg, uint32_t k, const BzgBase *base, uint32_t rows, const uint64_t *totals, uint64_t *out)
{
    const BzgmSeg &s = seg[k];
    uint64_t *o = out + (size_t)k * BZGM_TOTALS;
    if (!s.rows) {
        o[BZGM_T_RECORDS] = o[BZGM_T_SEL] = o[BZGM_T_BYTES] = 0;
        return;
    }
    const uint32_t end = s.first + s.rows;
    const BzgBase a = base[s.first];
    const BzgBase b = end < rows ? base[end] : BzgBase{totals[BZG_T_BYTES], totals[BZG_T_SEL], totals[BZG_T_DEL]};
    o[BZGM_T_RECORDS] = b.del - a.del, o[BZGM_T_SEL] = b.sel - a.sel, o[BZGM_T_BYTES] = b.out - a.out;
}

#endif // BZH_GREP_MANY_CORE_H
