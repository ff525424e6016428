// grep_ctx_core.h -- the grep with CONTEXT RECORDS (bzh_grep_set_context: grep -A -B -C), beside grep_core.h and in its style:
// what one thread and one tile of grep_ctx_tiles / grep_ctx_gather (grep.hip) do, and the two scans over the tiles between the
// passes.  Plain C++ phases of (tid, shared) without a launch in it: the kernels compile it for the device,
// tests/decode_host/grep_ctx_host.cpp for the host, against a naive split-find-dilate.
//
// THE RULE.  A record is PRIMARY when the plain grep selects it.  With before = B and after = A, record r is SELECTED when a
// primary p has p - B <= r <= p + A.  Both halves are DISTANCES over records: `back`, the records closed since the last primary
// (0: the record is primary), and `next`, the records up to the next primary.  r is selected when back <= A or next <= B.  A
// distance saturates ("none within reach"), so any uint32_t A and B is taken, in 64-bit sums.
//
// THE PASSES.  A tile cannot know the bytes it selects before it knows the two distances at its edges, and those are known only
// after a scan over all tiles.  So there are three passes over the tiles and two scans:
//   pass one   (the matcher runs here and only here)  every thread's hit starts go to a table, 16 bits a thread; the tile's
//              record: its delimiters, and how many lie in front of its first and behind its last primary (BzcTile)
//   scan one   forward: the hit state, the open record's start and `back` at every tile's entry; backward: `next` at its exit
//   pass two   the selection of every record of the tile: its selected bytes, records, context records and groups (BzcCount);
//              the one thread of the window that holds the first PENDING record's start stores it
//   scan two   the sums in front of every tile
//   gather     the selection again, the compaction in LDS and the entries as grep_core.h's, bit 63 of len on context records
// Passes two and three read the hit table, not the pattern.  No atomics; every workgroup copies only bytes of its own tile.
//
// THE WINDOW (BzcWindow).  As BzgWindow, and in front of the open record the PENDING RECORDS [q_lo, t_lo): closed records of
// earlier windows that are not primary -- that is final -- and that a primary of this window may still select.  Their delimiters
// are seen, for bytes, entries and numbering; no match is sought in them.
#ifndef BZH_GREP_CTX_CORE_H
#define BZH_GREP_CTX_CORE_H
#include "grep_core.h"

#define BZC_LEN_CONTEXT (1ull << 63) // BZH_GREP_LEN_CONTEXT

struct BzcWindow {
    BzgWindow w;      // t_lo: where the open record begins; rec_base: the records closed in front of q_lo
    uint64_t q_lo;    // the pending records begin here: q_lo <= t_lo
    uint64_t back_in; // records closed since the last primary, in front of q_lo (saturated)
    uint64_t sat_a;   // after + before + 1: where `back` saturates ("beyond every reach"; also: no primary so far)
    uint64_t sat_b;   // before + 1: where `next` saturates
    uint32_t before, after;
    uint32_t last;    // the finishing window: a primary tail selects the records in front of it
};

enum : uint32_t { BZC_HAS_PRIM = 16, BZC_HEAD_PRIM = 32, BZC_OPEN_END = 64 }; // beside BZG_HEAD_HIT, BZG_TAIL_HIT
struct BzcTile {
    uint32_t nd, fl;     // as BzgTile's
    uint32_t flags;      // pass one: HEAD_HIT, TAIL_HIT, HAS_PRIM (a primary among the records behind the first delimiter).  Scan
                         // one: HEAD_PRIM (the record that ends at the first delimiter is primary), OPEN_END (the record that
                         // leaves the tile open is not closed in this window)
    uint32_t np;         // primaries behind the first delimiter
    uint32_t fp, la;     // delimiters in front of the first of them, and behind the last
    uint64_t open_start; // scan one: where the record that is open at the tile's first byte begins
    uint64_t back;       // ... the records closed since the last primary, at the tile's entry
    uint64_t next;       // ... the distance from the record that leaves the tile open to the next primary (0: it is one)
};
struct BzcCount { // pass two
    uint32_t bytes, sel, ctx, groups;
};
enum : uint32_t {
    BZC_T_CTX = BZG_TOTALS, // context records
    BZC_T_GROUPS,
    BZC_T_PRIM,       // primary records
    BZC_T_BACK,       // `back` behind the window's last delimiter
    BZC_T_PEND_N,     // the records that stay pending
    BZC_T_PEND_START, // where they begin
    BZC_T_PEND_FIND,  // scan one to pass two: PEND_N if a thread has to find PEND_START, else ~0
    BZC_TOTALS
};
BZF_FN uint64_t bzc_sat(uint64_t v, uint64_t at) { return v < at ? v : at; }

// ---- the two distance scans of a workgroup, in the shape of bzg_step_f/b ------------------------------------------------------
// an element: bit 31 "a primary", bits 0 .. 12 the delimiters behind the last one (forward) / in front of the first one (backward),
// or without a primary all delimiters
enum : uint32_t { BZC_HAS = 1u << 31, BZC_CNT = 0xFFFFu };
struct BzcShared {
    BzgShared g;
    uint32_t cf[2][BZF_THREADS];
    uint32_t cb[2][BZF_THREADS];
};
BZF_FN void bzc_step(BzcShared &sh, uint32_t tid, uint32_t k)
{
    const uint32_t off = 1u << k, *f = sh.cf[k & 1u], *b = sh.cb[k & 1u];
    sh.cf[~k & 1u][tid] = tid >= off ? ((f[tid] & BZC_HAS) ? f[tid] : f[tid - off] + f[tid]) : f[tid];
    sh.cb[~k & 1u][tid] = tid + off < BZF_THREADS ? ((b[tid] & BZC_HAS) ? b[tid] : b[tid + off] + b[tid]) : b[tid];
}
// four sums of at most 4,096 in 16 bits each
BZF_FN uint64_t bzc_pack(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return (uint64_t)a | (uint64_t)b << 16 | (uint64_t)c << 32 | (uint64_t)d << 48; }
BZF_FN uint32_t bzc_get(uint64_t v, uint32_t j) { return (uint32_t)(v >> (16 * j)) & 0xFFFFu; }

// ---- one thread -----------------------------------------------------------------------------------------------------------------
// its masks: the delimiters of [q_lo, p_hi), the bytes the window may emit; hm: the matcher's hit starts.  A match that started
// in the processed part of the carry is a hit start at t_lo, so that the pending records in front of it do not inherit it
BZF_FN void bzc_masks(BzgThread &t, const BzcWindow &w, uint64_t p0, const BzfVec &own, uint32_t delim, uint32_t hm)
{
    t.dm = bzf_eq_mask16(own.x, own.y, own.z, own.w, delim) & bzf_range_mask16(p0, w.q_lo, w.w.p_hi);
    t.hm = hm | (w.w.open_hit ? bzf_range_mask16(p0, w.w.t_lo, w.w.t_lo + 1) : 0u);
    t.vm = bzf_range_mask16(p0, w.q_lo, w.w.p_hi);
    t.first = t.last = 0;
    t.loc_sm = t.loc_sdm = t.loc_bytes = 0;
    if (t.dm) t.first = bzg_ctz(t.dm), t.last = bzg_top(t.dm);
}
// the primaries among the records that end at the thread's delimiters.  e: the forward scan in front of the thread; head: whether
// the tile's head record is primary (pass one does not know: false).  *is_head: the thread's first delimiter is the tile's first,
// *head_hit: that record's hit starts in this tile
BZF_FN uint32_t bzc_prim(const BzgThread &t, const BzcWindow &w, uint64_t p0, uint32_t e, bool head, bool *is_head, bool *head_hit)
{
    *is_head = *head_hit = false;
    if (!t.dm) return 0u;
    uint32_t pm = 0, rest = t.dm & (t.dm - 1u), prev = t.first;
    while (rest) {
        const uint32_t k = bzg_ctz(rest), seg = bzg_upto(k) & ~bzg_upto(prev); // (prev, k]
        rest &= rest - 1u;
        if (((t.hm & seg) != 0) != (w.w.invert != 0)) pm |= 1u << k;
        prev = k;
    }
    bool s;
    if (bzg_first(t, e, w.w.invert, &s)) {
        if (s) pm |= 1u << t.first;
    } else {
        *is_head = true, *head_hit = s;
        if (head) pm |= 1u << t.first;
    }
    return pm & bzf_range_mask16(p0, w.w.t_lo, w.w.p_hi); // (a pending record is not primary)
}
BZF_FN uint32_t bzc_fwd_elem(uint32_t dm, uint32_t pm)
{
    return pm ? BZC_HAS | (uint32_t)__builtin_popcount(dm & ~bzg_upto(bzg_top(pm))) : (uint32_t)__builtin_popcount(dm);
}
BZF_FN uint32_t bzc_bwd_elem(uint32_t dm, uint32_t pm)
{
    return pm ? BZC_HAS | (uint32_t)__builtin_popcount(dm & bzg_below(bzg_ctz(pm))) : (uint32_t)__builtin_popcount(dm);
}

// ---- pass one: a tile's record ------------------------------------------------------------------------------------------------------
// phase 0: bzg_count_p0 and bzg_step_f 0 .. 7 on sh.g.  phase 1: the primaries, the elements of the three scans; then bzc_step and
// bzg_step_s 0 .. 7
BZF_FN void bzc_count_p1(BzcShared &sh, uint32_t tid, const BzgThread &t, const BzcWindow &w, uint64_t p0)
{
    bool is_head, head_hit;
    const uint32_t pm = bzc_prim(t, w, p0, tid ? sh.g.f[0][tid - 1] : 0u, false, &is_head, &head_hit);
    if (is_head) sh.g.head = (head_hit ? BZG_HEAD_HIT : 0u) | (tid * BZF_ITEMS + t.first) << 16; // (one thread of the tile)
    sh.cf[0][tid] = bzc_fwd_elem(t.dm, pm), sh.cb[0][tid] = bzc_bwd_elem(t.dm, pm);
    sh.g.s[0][tid] = bzg_pack(0, (uint32_t)__builtin_popcount(pm), (uint32_t)__builtin_popcount(t.dm));
}
// phase 2, one thread
BZF_FN void bzc_count_p2(const BzcShared &sh, BzcTile &out)
{
    const uint32_t all = sh.g.f[0][BZF_THREADS - 1], cf = sh.cf[0][BZF_THREADS - 1], cb = sh.cb[0][0];
    const uint64_t sum = sh.g.s[0][BZF_THREADS - 1];
    out.nd = bzg_del(sum), out.np = bzg_sel(sum);
    out.fp = cb & BZC_CNT, out.la = cf & BZC_CNT;
    out.open_start = out.back = out.next = 0;
    if (all & BZG_F_DEL) {
        out.fl = (sh.g.head >> 16) | (all & BZG_F_POS) << 16;
        out.flags = (sh.g.head & BZG_HEAD_HIT) | ((all & BZG_F_HIT) ? BZG_TAIL_HIT : 0u) | ((cf & BZC_HAS) ? BZC_HAS_PRIM : 0u);
    } else {
        out.fl = 0;
        out.flags = (all & BZG_F_HIT) ? (BZG_HEAD_HIT | BZG_TAIL_HIT) : 0u;
    }
}

// ---- scan one: the distances at every tile's edges (chunks as grep_scan's: bzg_chunk) -----------------------------------------------
struct BzcFwd { // in front of a tile
    uint32_t hit;   // a hit start in the open record
    uint64_t start; // where it begins
    uint64_t back;  // records closed since the last primary
    uint64_t del;   // delimiters
};
// the state behind tile t from the one in front of it; returns whether its head record is primary
BZF_FN bool bzc_tile_fwd(const BzcTile &x, uint32_t t, const BzcWindow &w, BzcFwd &s)
{
    if (!x.nd) {
        s.hit |= (x.flags & BZG_HEAD_HIT) != 0;
        return false;
    }
    const uint64_t t0 = (uint64_t)t * BZF_TILE;
    const bool head = ((s.hit || (x.flags & BZG_HEAD_HIT)) != (w.w.invert != 0)) && t0 + (x.fl & 0xFFFFu) >= w.w.t_lo;
    if (x.flags & BZC_HAS_PRIM) s.back = x.la;
    else if (head) s.back = x.nd - 1;
    else s.back = bzc_sat(s.back + x.nd, w.sat_a);
    s.hit = (x.flags & BZG_TAIL_HIT) != 0;
    s.start = t0 + (x.fl >> 16) + 1;
    s.del += x.nd;
    return head;
}
// `next` of the record that enters tile x open, from that of the one that leaves it open
BZF_FN uint64_t bzc_tile_bwd(const BzcTile &x, uint64_t next, const BzcWindow &w)
{
    if (!x.nd) return next;
    if (x.flags & BZC_HEAD_PRIM) return 0;
    if (x.flags & BZC_HAS_PRIM) return x.fp;
    return bzc_sat(next + x.nd, w.sat_b);
}
struct BzcScanShared {
    // forward, a chunk: bit 0 "it holds a delimiter", bit 1 the hit state behind it (without a delimiter: a hit), bit 2 "its first
    // delimiter is pending", bit 3 "a hit in front of its first delimiter", bit 4 "a primary whatever enters"; then the hit state
    // in front of it
    uint32_t h[BZF_THREADS];
    uint64_t s[BZF_THREADS];  // the open record's start behind it; then in front of it
    uint64_t n[BZF_THREADS];  // its delimiters; then those in front of it
    uint64_t a[BZF_THREADS];  // the delimiters behind its last primary (bit 4), else as n; then `back` in front of it
    // backward, a chunk: bit 0 "it holds a delimiter", bit 1 "a primary"; then "no delimiter behind it"
    uint32_t b[BZF_THREADS];
    uint64_t p[BZF_THREADS];  // the delimiters in front of its first primary; then `next` behind it
    uint64_t np[BZF_THREADS]; // its primaries
    uint32_t tail_prim;       // the finishing window's tail is a primary record
};
// phase A: the chunks forward, whatever enters them
BZF_FN void bzc_scan_a(BzcScanShared &sh, uint32_t tid, const BzcTile *tile, uint32_t tiles, const BzcWindow &w)
{
    uint32_t lo, hi, any = 0, pend = 0, hh = 0, known = 0;
    BzcFwd s{0, 0, 0, 0};
    BzcWindow never = w, plain = w;
    never.w.invert = 0;                      // (no hit, not inverted: not primary)
    never.sat_a = plain.sat_a = ~0ull;       // (sums of at most 2^32 delimiters; saturated in phase B)
    bzg_chunk(tid, tiles, &lo, &hi);
    for (uint32_t t = lo; t < hi; t++) {
        const BzcTile x = tile[t];
        if (!any && x.nd) { // the chunk's first delimiter: whether its record is primary depends on what enters
            any = 1, hh = s.hit | ((x.flags & BZG_HEAD_HIT) != 0), pend = (uint64_t)t * BZF_TILE + (x.fl & 0xFFFFu) < w.w.t_lo;
            s.hit = 0;
            BzcTile y = x;
            y.flags &= ~(uint32_t)BZG_HEAD_HIT;
            bzc_tile_fwd(y, t, never, s);
            known = (x.flags & BZC_HAS_PRIM) != 0;
            continue;
        }
        const bool head = bzc_tile_fwd(x, t, plain, s);
        known |= x.nd && (head || (x.flags & BZC_HAS_PRIM));
    }
    sh.h[tid] = any | s.hit << 1 | pend << 2 | hh << 3 | known << 4;
    sh.s[tid] = s.start, sh.n[tid] = s.del, sh.a[tid] = s.back;
}
// phase B, one thread: the state in front of every chunk; the tail of the window and the records that stay pending
BZF_FN void bzc_scan_b(BzcScanShared &sh, const BzcWindow &w, uint64_t *totals)
{
    BzcFwd s{0, w.q_lo, w.back_in, 0};
    for (uint32_t k = 0; k < BZF_THREADS; k++) {
        const uint32_t h = sh.h[k];
        const uint64_t start = sh.s[k], n = sh.n[k], a = sh.a[k];
        sh.h[k] = s.hit, sh.s[k] = s.start, sh.n[k] = s.del, sh.a[k] = s.back;
        if (h & 1u) {
            const bool head = ((s.hit || (h & 8u)) != (w.w.invert != 0)) && !(h & 4u);
            s.back = bzc_sat((h & 16u) ? a : head ? n - 1 : s.back + n, w.sat_a);
            s.hit = (h >> 1) & 1u, s.start = start, s.del += n;
        } else {
            s.hit |= (h >> 1) & 1u;
        }
    }
    sh.tail_prim = w.last && s.start < w.w.n && (s.hit != 0) != (w.w.invert != 0);
    // the closed records that a later primary may still select: beyond the reach of the last primary, and the last `before` of those
    uint64_t keep = w.last || s.back <= w.after ? 0 : s.back - w.after;
    if (keep > w.before) keep = w.before;
    if (keep > s.del) keep = s.del;
    totals[BZG_T_DEL] = s.del, totals[BZG_T_TAIL_START] = s.start, totals[BZG_T_TAIL_HIT] = s.hit;
    totals[BZC_T_BACK] = s.back, totals[BZC_T_PEND_N] = keep;
    totals[BZC_T_PEND_START] = keep == s.del ? w.q_lo : s.start; // (keep == 0: none; else a thread of pass two stores it)
    totals[BZC_T_PEND_FIND] = keep && keep < s.del ? keep : ~0ull;
}
// phase C: HEAD_PRIM, open_start, back and the delimiters in front of every tile; the chunks backward
BZF_FN void bzc_scan_c(BzcScanShared &sh, uint32_t tid, BzcTile *tile, uint32_t tiles, const BzcWindow &w, BzgBase *base)
{
    uint32_t lo, hi, has = 0;
    uint64_t cnt = 0, fp = 0, np = 0;
    BzcFwd s{sh.h[tid], sh.s[tid], sh.a[tid], sh.n[tid]};
    bzg_chunk(tid, tiles, &lo, &hi);
    for (uint32_t t = lo; t < hi; t++) {
        BzcTile x = tile[t];
        x.open_start = s.start, x.back = s.back;
        base[t].del = s.del;
        const bool head = bzc_tile_fwd(x, t, w, s);
        x.flags = (x.flags & (BZG_HEAD_HIT | BZG_TAIL_HIT | BZC_HAS_PRIM)) | (head ? BZC_HEAD_PRIM : 0u);
        tile[t] = x;
        if (!has && x.nd && (head || (x.flags & BZC_HAS_PRIM))) has = 1, fp = cnt + (head ? 0u : x.fp);
        cnt += x.nd, np += x.np + (head ? 1u : 0u);
    }
    sh.b[tid] = (cnt != 0) | has << 1;
    sh.p[tid] = has ? fp : cnt, sh.np[tid] = np;
}
// phase D, one thread: `next` behind every chunk
BZF_FN void bzc_scan_d(BzcScanShared &sh, const BzcWindow &w, uint64_t *totals)
{
    uint64_t next = sh.tail_prim ? 0 : w.sat_b, np = 0;
    uint32_t open = 1;
    for (uint32_t k = BZF_THREADS; k-- > 0;) {
        const uint32_t b = sh.b[k];
        const uint64_t p = sh.p[k];
        sh.b[k] = open, sh.p[k] = next;
        np += sh.np[k];
        if (b & 1u) open = 0, next = (b & 2u) ? p : bzc_sat(next + p, w.sat_b);
    }
    totals[BZC_T_PRIM] = np;
}
// phase E: next and OPEN_END of every tile
BZF_FN void bzc_scan_e(const BzcScanShared &sh, uint32_t tid, BzcTile *tile, uint32_t tiles, const BzcWindow &w)
{
    uint32_t lo, hi, open = sh.b[tid];
    uint64_t next = sh.p[tid];
    bzg_chunk(tid, tiles, &lo, &hi);
    for (uint32_t t = hi; t-- > lo;) {
        const BzcTile x = tile[t];
        tile[t].next = next;
        if (open) tile[t].flags = x.flags | BZC_OPEN_END;
        if (x.nd) open = 0;
        next = bzc_tile_bwd(x, next, w);
    }
}

// ---- passes two and three: the selection of a thread's records ------------------------------------------------------------------------
struct BzcSel {
    uint32_t sm;     // its selected bytes
    uint32_t sdm;    // the delimiters of its selected records,
    uint32_t cdm;    // ... of those that are context records
    uint32_t groups; // selected records of its own whose predecessor is not selected
};
// phase 1 (behind the forward scan): the elements of the distance scans; then bzc_step 0 .. 7.  Returns the thread's primaries
BZF_FN uint32_t bzc_sel_p1(BzcShared &sh, uint32_t tid, const BzgThread &t, const BzcTile &x, const BzcWindow &w, uint64_t p0)
{
    bool is_head, head_hit;
    const uint32_t pm = bzc_prim(t, w, p0, tid ? sh.g.f[0][tid - 1] : 0u, (x.flags & BZC_HEAD_PRIM) != 0, &is_head, &head_hit);
    sh.cf[0][tid] = bzc_fwd_elem(t.dm, pm), sh.cb[0][tid] = bzc_bwd_elem(t.dm, pm);
    return pm;
}
// phase 2: every record of the thread judged by its two distances.  first_rec: no record is closed in front of the tile.
// find: BZC_T_PEND_FIND; del_behind: the window's delimiters behind the tile; *pend_start: set by the one thread that holds the
// delimiter with exactly `find` delimiters behind it
BZF_FN BzcSel bzc_sel_p2(const BzcShared &sh, uint32_t tid, const BzgThread &t, uint32_t pm, const BzcTile &x, const BzcWindow &w, bool first_rec,
                         uint64_t p0, uint64_t find, uint64_t del_behind, uint64_t *pend_start)
{
    const uint32_t ef = tid ? sh.cf[0][tid - 1] : 0u, eb = tid + 1 < BZF_THREADS ? sh.cb[0][tid + 1] : 0u;
    const uint64_t A = w.after, B = w.before;
    uint64_t back = (ef & BZC_HAS) ? (ef & BZC_CNT) : x.back + ef;                  // closed since the last primary, in front of the thread
    const uint64_t next_x = (eb & BZC_HAS) ? (eb & BZC_CNT) : x.next + eb;          // of the record that is open behind its last delimiter
    const bool closes = (eb & (BZC_HAS | BZC_CNT)) != 0 || !(x.flags & BZC_OPEN_END); // ... which is closed in this window
    BzcSel r{0, 0, 0, 0};
    bool prev_sel = !(first_rec && !ef) && back <= A; // (the record in front: also next <= B, seen at the first delimiter)
    uint32_t prev = 0;
    bool any = false;
    for (uint32_t m = t.dm; m; m &= m - 1u) {
        const uint32_t k = bzg_ctz(m), ahead = pm & ~bzg_below(k), behind = (uint32_t)__builtin_popcount(t.dm & ~bzg_upto(k));
        const bool prim = (pm >> k) & 1u;
        back = prim ? 0 : back + 1;
        const uint64_t next = ahead ? (uint64_t)__builtin_popcount(t.dm & bzg_below(bzg_ctz(ahead)) & ~bzg_below(k)) : behind + 1 + next_x;
        const bool sel = back <= A || next <= B;
        if (!any && !(first_rec && !ef) && next + 1 <= B) prev_sel = true;
        if (sel) {
            r.sm |= any ? bzg_upto(k) & ~bzg_upto(prev) : bzg_upto(k);
            r.sdm |= 1u << k;
            if (!prim) r.cdm |= 1u << k;
            if (!prev_sel) r.groups++;
        }
        if (!(pm & ~bzg_upto(k)) && !(eb & BZC_HAS) && behind + (eb & BZC_CNT) + del_behind == find) *pend_start = p0 + k + 1;
        prev_sel = sel, prev = k, any = true;
    }
    if (closes && (back + 1 <= A || next_x <= B)) r.sm |= any ? 0xFFFFu & ~bzg_upto(prev) : 0xFFFFu;
    r.sm &= t.vm;
    return r;
}
// pass two, phase 3: the elements of the sums; then bzg_step_s 0 .. 7; phase 4, one thread: the tile's counts
BZF_FN void bzc_count2_p3(BzcShared &sh, uint32_t tid, const BzcSel &r)
{
    sh.g.s[0][tid] = bzc_pack((uint32_t)__builtin_popcount(r.sm), (uint32_t)__builtin_popcount(r.sdm), (uint32_t)__builtin_popcount(r.cdm), r.groups);
}
BZF_FN void bzc_count2_p4(const BzcShared &sh, BzcCount &out)
{
    const uint64_t v = sh.g.s[0][BZF_THREADS - 1];
    out.bytes = bzc_get(v, 0), out.sel = bzc_get(v, 1), out.ctx = bzc_get(v, 2), out.groups = bzc_get(v, 3);
}
// the gather, phase 3: the elements of bzg_gather_p3's sums; then bzg_step_s 0 .. 7, bzg_gather_p3 on sh.g, and phase 4: bit 63
// of len in the entries of the thread's context records (it has just stored them itself)
BZF_FN void bzc_gather_p3(BzcShared &sh, uint32_t tid, const BzgThread &t, const BzcSel &r)
{
    sh.g.s[0][tid] = bzg_pack((uint32_t)__builtin_popcount(r.sm), (uint32_t)__builtin_popcount(r.sdm), (uint32_t)__builtin_popcount(t.dm));
}
BZF_FN void bzc_gather_mark(const BzcShared &sh, uint32_t tid, const BzgBase &base, const BzcSel &r, BzgEntry *ent)
{
    if (!ent || !r.cdm) return;
    uint64_t rank = base.sel + bzg_sel(tid ? sh.g.s[0][tid - 1] : 0u);
    for (uint32_t m = r.sdm; m; m &= m - 1u, rank++)
        if (r.cdm & m & (0u - m)) ent[rank].len |= BZC_LEN_CONTEXT;
}

// ---- scan two: the sums in front of every tile ------------------------------------------------------------------------------------------
struct BzcSumShared {
    uint64_t c[4][BZF_THREADS]; // a chunk's selected bytes, selected records, context records, groups; then those in front of it
};
BZF_FN void bzc_sum_a(BzcSumShared &sh, uint32_t tid, const BzcCount *cnt, uint32_t tiles)
{
    uint32_t lo, hi;
    uint64_t r[4] = {0, 0, 0, 0};
    bzg_chunk(tid, tiles, &lo, &hi);
    for (uint32_t t = lo; t < hi; t++) r[0] += cnt[t].bytes, r[1] += cnt[t].sel, r[2] += cnt[t].ctx, r[3] += cnt[t].groups;
    for (uint32_t j = 0; j < 4; j++) sh.c[j][tid] = r[j];
}
BZF_FN void bzc_sum_b(BzcSumShared &sh, uint64_t *totals) // one thread
{
    uint64_t r[4] = {0, 0, 0, 0};
    for (uint32_t k = 0; k < BZF_THREADS; k++)
        for (uint32_t j = 0; j < 4; j++) {
            const uint64_t v = sh.c[j][k];
            sh.c[j][k] = r[j];
            r[j] += v;
        }
    totals[BZG_T_BYTES] = r[0], totals[BZG_T_SEL] = r[1], totals[BZC_T_CTX] = r[2], totals[BZC_T_GROUPS] = r[3];
}
BZF_FN void bzc_sum_c(const BzcSumShared &sh, uint32_t tid, const BzcCount *cnt, uint32_t tiles, BzgBase *base)
{
    uint32_t lo, hi;
    uint64_t bytes = sh.c[0][tid], sel = sh.c[1][tid];
    bzg_chunk(tid, tiles, &lo, &hi);
    for (uint32_t t = lo; t < hi; t++) {
        base[t].out = bytes, base[t].sel = sel;
        bytes += cnt[t].bytes, sel += cnt[t].sel;
    }
}

#endif // BZH_GREP_CTX_CORE_H
