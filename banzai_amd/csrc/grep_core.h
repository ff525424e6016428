// grep_core.h -- what ONE THREAD and ONE TILE of grep_tiles (grep.hip) do, and the scan between the two passes (grep_scan): which
// records of a window hold a match, and where their bytes go.  Plain C++ without a launch in it: the kernel compiles it for the
// device, tests/decode_host/grep_host.cpp for the host, where it runs thread by thread and tile by tile in the kernel's layout
// against a naive split-and-find.  The tile front -- the load, the staging, the filter and the verify -- and the masks of a
// thread's 16 bytes are search_core.h's; what is here begins with a thread's hit starts and delimiters.
//
// THE WINDOW.  Positions are in the coordinates of the buffer the kernel is given (BzgWindow).  The text is [t_lo, n) and begins at
// a record start.  A window PROCESSES the positions [p_lo, p_hi): their delimiters close records, and matches that start there are
// found (s_hi = min(p_hi, n - plen + 1): a match ends inside the text).  [t_lo, p_lo) was processed by earlier windows and holds no
// delimiter; open_hit says whether a match started there.  [p_hi, n) is left to the next window: a match that starts there may end
// behind n, and a pattern may hold the delimiter, so the records that end there cannot be judged yet.
//
// THE WORK.  Every thread knows the hit starts (hm) and the delimiters (dm) among its 16 positions.  A forward segmented scan over
// the workgroup gives it what lies between the last delimiter in front of it and itself; a backward one, in the gather, whether
// the record its last bytes belong to is selected.  What a tile cannot know -- the record that enters it, the record that leaves
// it -- is settled by the scan over the tiles.  Every workgroup counts and copies only bytes of its own tile.
//
// A workgroup-wide step is written as PHASES: functions of (tid, shared) that read what the phase before wrote.  The kernel runs a
// phase in every thread and then a barrier; the host runs it for tid = 0 .. 255 in a loop.
#ifndef BZH_GREP_CORE_H
#define BZH_GREP_CORE_H
#include "search_core.h"

struct BzgWindow {
    uint64_t n;          // bytes [0, n) of the buffer may be read (to the aligned word that holds byte n - 1)
    uint64_t t_lo;       // the open record begins here: t_lo <= p_lo
    uint64_t p_lo, p_hi; // the positions this window processes
    uint64_t s_hi;       // hit starts: [p_lo, s_hi)
    uint64_t off_base;   // output offset of position p: off_base + p (modulo 2^64)
    uint64_t rec_base;   // records closed in front of the window
    uint64_t out_base;   // selected bytes in front of the window
    uint64_t sel_base;   // selected records in front of the window
    uint32_t open_hit;   // a match started in [t_lo, p_lo)
    uint32_t invert;
};

enum : uint32_t { BZG_HEAD_HIT = 1, BZG_TAIL_HIT = 2, BZG_SEL_END = 4, BZG_SEL_TAIL = 8 };
struct BzgTile { // pass one, then the scan
    uint32_t nd;          // delimiters
    uint32_t fl;          // tile positions of the first and the last of them: first | last << 16
    uint32_t flags;       // pass one: HEAD_HIT (a hit start at or in front of the first delimiter), TAIL_HIT (behind the last);
                          // without a delimiter both say "a hit".  The scan: SEL_END (the record that ends at the first
                          // delimiter is selected), SEL_TAIL (the record that leaves the tile open is, decided in a later tile)
    uint32_t inner_sel;   // records wholly inside the tile: the selected ones,
    uint32_t inner_bytes; // ... and their bytes
    uint32_t bytes;       // the scan: selected bytes of the tile
    uint64_t open_start;  // the scan: where the record that is open at the tile's first byte begins
};
struct BzgBase { // the scan: in front of every tile, within the window
    uint64_t out, sel, del; // selected bytes, selected records, delimiters
};
struct BzgEntry { // bzh_grep_entry
    uint64_t record, off, len, out_off;
};
enum : uint32_t { BZG_T_SEL = 0, BZG_T_BYTES = 1, BZG_T_DEL = 2, BZG_T_TAIL_START = 3, BZG_T_TAIL_HIT = 4, BZG_TOTALS = 5 };

// ---- the scans of a workgroup: Hillis-Steele over an array of BZF_THREADS elements in two buffers, 8 steps ---------------------
// forward segmented: bit 31 "a delimiter", bit 30 "a hit start behind the last delimiter", bits 0 .. 11 the last delimiter's place
enum : uint32_t { BZG_F_DEL = 1u << 31, BZG_F_HIT = 1u << 30, BZG_F_POS = 0xFFFu };
BZF_FN uint32_t bzg_fwd(uint32_t a, uint32_t b) { return (b & BZG_F_DEL) ? b : (a | (b & BZG_F_HIT)); }
// backward "the nearest behind": bit 1 "a delimiter", bit 0 "its record is selected"
BZF_FN uint32_t bzg_bwd(uint32_t near, uint32_t far) { return (near & 2u) ? near : far; }
// three sums of at most 4,096 in 20 bits each: selected bytes, selected records, delimiters
BZF_FN uint64_t bzg_pack(uint32_t bytes, uint32_t sel, uint32_t del) { return (uint64_t)bytes | (uint64_t)sel << 20 | (uint64_t)del << 40; }
BZF_FN uint32_t bzg_bytes(uint64_t v) { return (uint32_t)v & 0xFFFFFu; }
BZF_FN uint32_t bzg_sel(uint64_t v) { return (uint32_t)(v >> 20) & 0xFFFFFu; }
BZF_FN uint32_t bzg_del(uint64_t v) { return (uint32_t)(v >> 40) & 0xFFFFFu; }

struct BzgShared {
    uint32_t f[2][BZF_THREADS];
    uint32_t b[2][BZF_THREADS];
    uint64_t s[2][BZF_THREADS];
    uint32_t head;                                             // the tile's head record: HEAD_HIT, and the first delimiter's place << 16
    __attribute__((aligned(16))) uint8_t cbuf[BZF_TILE + 16]; // the tile's selected bytes, shifted to the output's word alignment
};
// step k = 0 .. 7 of the three scans (src = buffer k & 1; the result of step 7 lies in buffer 0)
BZF_FN void bzg_step_f(BzgShared &sh, uint32_t tid, uint32_t k)
{
    const uint32_t off = 1u << k, *src = sh.f[k & 1u];
    sh.f[~k & 1u][tid] = tid >= off ? bzg_fwd(src[tid - off], src[tid]) : src[tid];
}
BZF_FN void bzg_step_b(BzgShared &sh, uint32_t tid, uint32_t k)
{
    const uint32_t off = 1u << k, *src = sh.b[k & 1u];
    sh.b[~k & 1u][tid] = tid + off < BZF_THREADS ? bzg_bwd(src[tid], src[tid + off]) : src[tid];
}
BZF_FN void bzg_step_s(BzgShared &sh, uint32_t tid, uint32_t k)
{
    const uint32_t off = 1u << k;
    const uint64_t *src = sh.s[k & 1u];
    sh.s[~k & 1u][tid] = tid >= off ? src[tid - off] + src[tid] : src[tid];
}

// ---- one thread --------------------------------------------------------------------------------------------------------------
BZF_FN uint32_t bzg_below(uint32_t k) { return (1u << k) - 1u; }      // bits 0 .. k - 1 (k <= 16)
BZF_FN uint32_t bzg_upto(uint32_t k) { return (2u << k) - 1u; }       // bits 0 .. k
BZF_FN uint32_t bzg_ctz(uint32_t v) { return (uint32_t)__builtin_ctz(v); }
BZF_FN uint32_t bzg_top(uint32_t v) { return 31u - (uint32_t)__builtin_clz(v); }

struct BzgThread {
    uint32_t hm, dm, vm;   // hit starts, delimiters, and the bytes of the text that this window may emit: [t_lo, p_hi)
    uint32_t first, last;  // places of its first and last delimiter (dm != 0)
    uint32_t loc_sm;       // the records between them: the bytes of the selected ones,
    uint32_t loc_sdm;      // ... their delimiters,
    uint32_t loc_bytes;    // ... and the sum of their lengths
};

// the masks of a thread's 16 bytes `own` at position p0 (hm: its hit starts, bzf_match16 under bzg_starts), and what it can say
// about its own bytes
BZF_FN uint32_t bzg_starts(const BzgWindow &w, uint64_t p0) { return bzf_range_mask16(p0, w.p_lo, w.s_hi); }
BZF_FN void bzg_masks(BzgThread &t, const BzgWindow &w, uint64_t p0, const BzfVec &own, uint32_t delim, uint32_t hm)
{
    t.dm = bzf_eq_mask16(own.x, own.y, own.z, own.w, delim) & bzf_range_mask16(p0, w.p_lo, w.p_hi);
    t.hm = hm;
    t.vm = bzf_range_mask16(p0, w.t_lo, w.p_hi);
}
BZF_FN void bzg_local(BzgThread &t, uint32_t invert)
{
    t.first = t.last = 0;
    t.loc_sm = t.loc_sdm = t.loc_bytes = 0;
    if (!t.dm) return;
    t.first = bzg_ctz(t.dm), t.last = bzg_top(t.dm);
    uint32_t rest = t.dm & (t.dm - 1u), prev = t.first;
    while (rest) {
        const uint32_t k = bzg_ctz(rest), seg = bzg_upto(k) & ~bzg_upto(prev); // (prev, k]
        rest &= rest - 1u;
        if (((t.hm & seg) != 0) != (invert != 0)) t.loc_sm |= seg, t.loc_sdm |= 1u << k, t.loc_bytes += k - prev;
        prev = k;
    }
}
// the thread's element of the forward scan: its last delimiter and the hit starts behind it, or without one its hit starts
BZF_FN uint32_t bzg_fwd_elem(const BzgThread &t, uint32_t tid)
{
    if (!t.dm) return t.hm ? BZG_F_HIT : 0u;
    return BZG_F_DEL | ((t.hm & ~bzg_upto(t.last)) ? BZG_F_HIT : 0u) | (tid * BZF_ITEMS + t.last);
}
// the record that ends at the thread's first delimiter (dm != 0), e: the forward scan in front of the thread.  Inside the tile
// (e has a delimiter): *sel whether it is selected, returns true.  Else it is the tile's head record: *sel = its hit starts in
// this tile, returns false.
BZF_FN bool bzg_first(const BzgThread &t, uint32_t e, uint32_t invert, bool *sel)
{
    const bool hit = (e & BZG_F_HIT) || (t.hm & bzg_upto(t.first));
    if (!(e & BZG_F_DEL)) {
        *sel = hit;
        return false;
    }
    *sel = hit != (invert != 0);
    return true;
}

// ---- pass one: a tile's record ---------------------------------------------------------------------------------------------------
// phase 0: the elements of the forward scan; then bzg_step_f 0 .. 7
BZF_FN void bzg_count_p0(BzgShared &sh, uint32_t tid, const BzgThread &t) { sh.f[0][tid] = bzg_fwd_elem(t, tid); }
// phase 1: the record at the thread's first delimiter, the elements of the sums; then bzg_step_s 0 .. 7
BZF_FN void bzg_count_p1(BzgShared &sh, uint32_t tid, const BzgThread &t, uint32_t invert)
{
    uint32_t sel = 0, bytes = t.loc_bytes;
    if (t.dm) {
        const uint32_t e = tid ? sh.f[0][tid - 1] : 0u;
        bool s;
        if (bzg_first(t, e, invert, &s)) {
            if (s) sel = 1, bytes += tid * BZF_ITEMS + t.first - (e & BZG_F_POS);
        } else {
            sh.head = (s ? BZG_HEAD_HIT : 0u) | (tid * BZF_ITEMS + t.first) << 16; // (one thread of the tile)
        }
    }
    sh.s[0][tid] = bzg_pack(bytes, sel + (uint32_t)__builtin_popcount(t.loc_sdm), (uint32_t)__builtin_popcount(t.dm));
}
// phase 2, one thread: the tile's record
BZF_FN void bzg_count_p2(const BzgShared &sh, BzgTile &out)
{
    const uint32_t all = sh.f[0][BZF_THREADS - 1];
    const uint64_t sum = sh.s[0][BZF_THREADS - 1];
    out.nd = bzg_del(sum);
    out.inner_sel = bzg_sel(sum);
    out.inner_bytes = bzg_bytes(sum);
    out.bytes = 0;
    out.open_start = 0;
    if (all & BZG_F_DEL) {
        out.fl = (sh.head >> 16) | (all & BZG_F_POS) << 16;
        out.flags = (sh.head & BZG_HEAD_HIT) | ((all & BZG_F_HIT) ? BZG_TAIL_HIT : 0u);
    } else {
        out.fl = 0;
        out.flags = (all & BZG_F_HIT) ? (BZG_HEAD_HIT | BZG_TAIL_HIT) : 0u;
    }
}

// ---- the scan over the tiles of a window: thread tid takes the tiles [tid c, tid c + c), c = ceil(tiles / threads) -----------------
struct BzgScanShared {
    uint32_t h[BZF_THREADS]; // forward: bit 1 "the chunk holds a delimiter", bit 0 its hit state; then the state in front of it
    uint64_t s[BZF_THREADS]; // forward: the open record's start, likewise
    uint32_t b[BZF_THREADS]; // backward: bit 1 "the chunk holds a delimiter", bit 0 SEL_END of its first; then SEL_TAIL behind it
    uint64_t c[3][BZF_THREADS]; // the chunk's selected bytes, selected records, delimiters; then those in front of it
};
// WHAT A ROW OF THE TABLE IS.  The scan walks a table of tiles in order; a policy says which tile of the buffer row t stands for,
// whether a text begins with it (a wall in front of it: the hit state and the open record start anew, at *start) or ends with it
// (a wall behind it: nothing behind it selects its tail), and the window its bytes are cut to.  BzgOneText, the default: the rows
// are the tiles of one window, and no wall stands between two.  (Many texts in one table: grep_many_core.h.)
#if defined(__HIPCC__)
#define BZG_MEM __host__ __device__ __forceinline__
#else
#define BZG_MEM inline
#endif
struct BzgOneText {
    BZG_MEM uint32_t tile_no(uint32_t t) const { return t; }
    BZG_MEM bool enters(uint32_t, uint64_t *) const { return false; }
    BZG_MEM bool leaves(uint32_t) const { return false; }
    BZG_MEM const BzgWindow &window(uint32_t, const BzgWindow &w, BzgWindow &) const { return w; }
};
// The walks over a chunk wait for memory, tile after tile, and one workgroup has nothing else to run meanwhile: they take
// BZG_BATCH tiles at a time, all loads first (the loops over a batch are unrolled, so a batch lies in registers).
enum : uint32_t { BZG_BATCH = 8 };
#if defined(__HIPCC__)
#define BZG_UNROLL _Pragma("unroll")
#else
#define BZG_UNROLL
#endif
BZF_FN void bzg_chunk(uint32_t tid, uint32_t tiles, uint32_t *lo, uint32_t *hi)
{
    const uint32_t c = (tiles + BZF_THREADS - 1) / BZF_THREADS;
    *lo = tid * c < tiles ? tid * c : tiles;
    *hi = *lo + c < tiles ? *lo + c : tiles;
}
// the hit state and the open record's start behind tile t, from those in front of it
BZF_FN void bzg_tile_fwd(const BzgTile &x, uint32_t t, uint32_t *hit, uint64_t *start)
{
    if (x.nd) {
        *hit = (x.flags & BZG_TAIL_HIT) != 0;
        *start = (uint64_t)t * BZF_TILE + (x.fl >> 16) + 1;
    } else {
        *hit |= (x.flags & BZG_HEAD_HIT) != 0;
    }
}
// phase A: the chunks forward
template <class R = BzgOneText>
BZF_FN void bzg_scan_a(BzgScanShared &sh, uint32_t tid, const BzgTile *tile, uint32_t tiles, const R &rows = R{})
{
    uint32_t lo, hi, hit = 0, any = 0;
    uint64_t start = 0;
    bzg_chunk(tid, tiles, &lo, &hi);
    for (uint32_t t0 = lo; t0 < hi; t0 += BZG_BATCH) {
        const uint32_t m = hi - t0 < BZG_BATCH ? hi - t0 : BZG_BATCH;
        BzgTile x[BZG_BATCH];
        BZG_UNROLL
        for (uint32_t j = 0; j < BZG_BATCH; j++)
            if (j < m) x[j] = tile[t0 + j];
        BZG_UNROLL
        for (uint32_t j = 0; j < BZG_BATCH; j++)
            if (j < m) {
                if (rows.enters(t0 + j, &start)) any = 1, hit = 0;
                any |= x[j].nd != 0;
                bzg_tile_fwd(x[j], rows.tile_no(t0 + j), &hit, &start);
            }
    }
    sh.h[tid] = any << 1 | hit, sh.s[tid] = start;
}
// phase B, one thread: the state in front of every chunk; the tail of the window
BZF_FN void bzg_scan_b(BzgScanShared &sh, const BzgWindow &w, uint64_t *totals)
{
    uint32_t hit = w.open_hit;
    uint64_t start = w.t_lo;
    for (uint32_t k = 0; k < BZF_THREADS; k++) {
        const uint32_t h = sh.h[k];
        const uint64_t s = sh.s[k];
        sh.h[k] = hit, sh.s[k] = start;
        if (h & 2u) hit = h & 1u, start = s;
        else hit |= h & 1u;
    }
    totals[BZG_T_TAIL_START] = start, totals[BZG_T_TAIL_HIT] = hit;
}
// phase C: SEL_END and open_start of every tile; the chunks backward
template <class R = BzgOneText>
BZF_FN void bzg_scan_c(BzgScanShared &sh, uint32_t tid, BzgTile *tile, uint32_t tiles, const BzgWindow &w, const R &rows = R{})
{
    uint32_t lo, hi, hit = sh.h[tid], back = 0;
    uint64_t start = sh.s[tid];
    bzg_chunk(tid, tiles, &lo, &hi);
    for (uint32_t t0 = lo; t0 < hi; t0 += BZG_BATCH) {
        const uint32_t m = hi - t0 < BZG_BATCH ? hi - t0 : BZG_BATCH;
        BzgTile x[BZG_BATCH];
        BZG_UNROLL
        for (uint32_t j = 0; j < BZG_BATCH; j++)
            if (j < m) x[j] = tile[t0 + j];
        BZG_UNROLL
        for (uint32_t j = 0; j < BZG_BATCH; j++)
            if (j < m) {
                if (rows.enters(t0 + j, &start)) hit = 0;
                uint32_t fl = x[j].flags & (BZG_HEAD_HIT | BZG_TAIL_HIT);
                if (x[j].nd) {
                    const bool sel = (hit || (fl & BZG_HEAD_HIT)) != (w.invert != 0);
                    if (sel) fl |= BZG_SEL_END;
                    if (!back) back = 2u | (sel ? 1u : 0u);
                }
                tile[t0 + j].open_start = start;
                tile[t0 + j].flags = fl;
                bzg_tile_fwd(x[j], rows.tile_no(t0 + j), &hit, &start);
            }
    }
    sh.b[tid] = back;
}
// phase D, one thread: SEL_TAIL behind every chunk (the window's last open record is not selected here: it is not closed)
BZF_FN void bzg_scan_d(BzgScanShared &sh)
{
    uint32_t cur = 0;
    for (uint32_t k = BZF_THREADS; k-- > 0;) {
        const uint32_t b = sh.b[k];
        sh.b[k] = cur;
        if (b & 2u) cur = b & 1u;
    }
}
// the tile's selected bytes: the head piece, the inner records, the tail piece, cut to what the window may emit
BZF_FN uint32_t bzg_tile_bytes(const BzgTile &x, uint32_t t, const BzgWindow &w)
{
    const uint64_t t0 = (uint64_t)t * BZF_TILE, t1 = t0 + BZF_TILE;
    const uint64_t lo = t0 > w.t_lo ? t0 : w.t_lo, hi = t1 < w.p_hi ? t1 : w.p_hi;
    if (!x.nd) return (x.flags & BZG_SEL_TAIL) && hi > lo ? (uint32_t)(hi - lo) : 0u;
    const uint64_t f = t0 + (x.fl & 0xFFFFu), l = t0 + (x.fl >> 16);
    uint32_t bytes = x.inner_bytes;
    if (x.flags & BZG_SEL_END) bytes += (uint32_t)(f + 1 - lo);
    if (x.flags & BZG_SEL_TAIL) bytes += (uint32_t)(hi - (l + 1));
    return bytes;
}
// phase E: SEL_TAIL and the bytes of every tile; the chunks' sums
template <class R = BzgOneText>
BZF_FN void bzg_scan_e(BzgScanShared &sh, uint32_t tid, BzgTile *tile, uint32_t tiles, const BzgWindow &w, const R &rows = R{})
{
    uint32_t lo, hi, cur = sh.b[tid];
    uint64_t bytes = 0, sel = 0, del = 0;
    bzg_chunk(tid, tiles, &lo, &hi);
    for (uint32_t t1 = hi; t1 > lo;) {
        const uint32_t m = t1 - lo < BZG_BATCH ? t1 - lo : BZG_BATCH, t0 = t1 - m;
        BzgTile x[BZG_BATCH];
        BZG_UNROLL
        for (uint32_t j = 0; j < BZG_BATCH; j++)
            if (j < m) x[j] = tile[t0 + j];
        BZG_UNROLL
        for (uint32_t j = BZG_BATCH; j-- > 0;)
            if (j < m) {
                if (rows.leaves(t0 + j)) cur = 0;
                if (cur) x[j].flags |= BZG_SEL_TAIL;
                if (x[j].nd) cur = (x[j].flags & BZG_SEL_END) != 0;
                BzgWindow cut;
                x[j].bytes = bzg_tile_bytes(x[j], rows.tile_no(t0 + j), rows.window(t0 + j, w, cut));
                tile[t0 + j].flags = x[j].flags;
                tile[t0 + j].bytes = x[j].bytes;
                bytes += x[j].bytes, sel += x[j].inner_sel + ((x[j].flags & BZG_SEL_END) ? 1u : 0u), del += x[j].nd;
            }
        t1 = t0;
    }
    sh.c[0][tid] = bytes, sh.c[1][tid] = sel, sh.c[2][tid] = del;
}
// phase F, one thread: the sums in front of every chunk, the window's totals
BZF_FN void bzg_scan_f(BzgScanShared &sh, uint64_t *totals)
{
    uint64_t r[3] = {0, 0, 0};
    for (uint32_t k = 0; k < BZF_THREADS; k++)
        for (uint32_t j = 0; j < 3; j++) {
            const uint64_t v = sh.c[j][k];
            sh.c[j][k] = r[j];
            r[j] += v;
        }
    totals[BZG_T_BYTES] = r[0], totals[BZG_T_SEL] = r[1], totals[BZG_T_DEL] = r[2];
}
// phase G: the sums in front of every tile
BZF_FN void bzg_scan_g(const BzgScanShared &sh, uint32_t tid, const BzgTile *tile, uint32_t tiles, BzgBase *base)
{
    uint32_t lo, hi;
    uint64_t bytes = sh.c[0][tid], sel = sh.c[1][tid], del = sh.c[2][tid];
    bzg_chunk(tid, tiles, &lo, &hi);
    for (uint32_t t0 = lo; t0 < hi; t0 += BZG_BATCH) {
        const uint32_t m = hi - t0 < BZG_BATCH ? hi - t0 : BZG_BATCH;
        BzgTile x[BZG_BATCH];
        BZG_UNROLL
        for (uint32_t j = 0; j < BZG_BATCH; j++)
            if (j < m) x[j] = tile[t0 + j];
        BZG_UNROLL
        for (uint32_t j = 0; j < BZG_BATCH; j++)
            if (j < m) {
                base[t0 + j] = BzgBase{bytes, sel, del};
                bytes += x[j].bytes, sel += x[j].inner_sel + ((x[j].flags & BZG_SEL_END) ? 1u : 0u), del += x[j].nd;
            }
    }
}

// ---- pass two: the gather of a tile that holds selected bytes ----------------------------------------------------------------------
// phase 0: as pass one.  phase 1: the element of the backward scan -- whether the record at the thread's first delimiter is
// selected; then bzg_step_b 0 .. 7
BZF_FN void bzg_gather_p1(BzgShared &sh, uint32_t tid, const BzgThread &t, const BzgTile &x, uint32_t invert, bool *sel_first)
{
    *sel_first = false;
    if (t.dm) {
        bool s;
        if (bzg_first(t, tid ? sh.f[0][tid - 1] : 0u, invert, &s)) *sel_first = s;
        else *sel_first = (x.flags & BZG_SEL_END) != 0;
    }
    sh.b[0][tid] = t.dm ? (2u | (*sel_first ? 1u : 0u)) : 0u;
}
// phase 2: the thread's selected bytes (*sm) and selected delimiters (*sdm), the elements of the sums; then bzg_step_s 0 .. 7
BZF_FN void bzg_gather_p2(BzgShared &sh, uint32_t tid, const BzgThread &t, const BzgTile &x, bool sel_first, uint32_t *sm, uint32_t *sdm)
{
    const uint32_t behind = tid + 1 < BZF_THREADS ? sh.b[0][tid + 1] : 0u;
    const bool sel_next = (behind & 2u) ? (behind & 1u) != 0 : (x.flags & BZG_SEL_TAIL) != 0;
    uint32_t m = t.loc_sm, d = t.loc_sdm;
    if (t.dm) {
        if (sel_first) m |= bzg_upto(t.first), d |= 1u << t.first;
        if (sel_next) m |= 0xFFFFu & ~bzg_upto(t.last);
    } else if (sel_next) {
        m = 0xFFFFu;
    }
    *sm = m & t.vm, *sdm = d;
    sh.s[0][tid] = bzg_pack((uint32_t)__builtin_popcount(*sm), (uint32_t)__builtin_popcount(d), (uint32_t)__builtin_popcount(t.dm));
}
// phase 3: the thread's selected bytes into cbuf (shift: the output address of the tile's first byte, modulo 4), its entries into
// ent (null: none are asked for; the window's slots [0, totals[SEL])).  own: the thread's 16 bytes, 4-byte aligned
BZF_FN void bzg_gather_p3(BzgShared &sh, uint32_t tid, uint32_t tile_no, const BzgThread &t, const BzgTile &x, const BzgBase &base,
                          const BzgWindow &w, const uint8_t *own, uint32_t sm, uint32_t sdm, uint32_t shift, bool bytes_wanted, BzgEntry *ent)
{
    const uint64_t ex = tid ? sh.s[0][tid - 1] : 0u;
    const uint32_t o = bzg_bytes(ex);
    if (bytes_wanted && sm) {
        uint8_t *to = sh.cbuf + shift + o;
        if (sm == 0xFFFFu && ((shift + o) & 3u) == 0) {
            const uint32_t *fw = reinterpret_cast<const uint32_t *>(own);
            uint32_t *tw = reinterpret_cast<uint32_t *>(to);
            tw[0] = fw[0], tw[1] = fw[1], tw[2] = fw[2], tw[3] = fw[3];
        } else {
            for (uint32_t m = sm; m; m &= m - 1u) *to++ = own[bzg_ctz(m)];
        }
    }
    if (!ent || !sdm) return;
    const uint64_t t0 = (uint64_t)tile_no * BZF_TILE, p0 = t0 + tid * BZF_ITEMS;
    uint64_t rank = base.sel + bzg_sel(ex);
    for (uint32_t m = sdm; m; m &= m - 1u) {
        const uint32_t k = bzg_ctz(m), before = t.dm & bzg_below(k);
        uint64_t start;
        if (before) {
            start = p0 + bzg_top(before) + 1;
        } else {
            const uint32_t e = tid ? sh.f[0][tid - 1] : 0u;
            start = (e & BZG_F_DEL) ? t0 + (e & BZG_F_POS) + 1 : x.open_start;
        }
        const uint64_t len = p0 + k + 1 - start;
        const uint64_t at = w.out_base + base.out + o + (uint32_t)__builtin_popcount(sm & bzg_below(k)); // (of the delimiter)
        ent[rank++] = BzgEntry{w.rec_base + base.del + bzg_del(ex) + (uint32_t)__builtin_popcount(before), w.off_base + start, len, at + 1 - len};
    }
}
// phase 4: cbuf[shift, shift + len) to dst[0, len) -- (dst - shift) is 4-byte aligned: words inside, bytes at the two ends
BZF_FN void bzg_gather_p4(const BzgShared &sh, uint32_t tid, uint8_t *dst, uint32_t shift, uint32_t len)
{
    const uint32_t end = shift + len, words = (end + 3u) / 4u;
    for (uint32_t j = tid; j < words; j += BZF_THREADS) {
        const uint32_t c0 = 4u * j;
        if (c0 >= shift && c0 + 4u <= end) {
            *reinterpret_cast<uint32_t *>(dst + c0 - shift) = *reinterpret_cast<const uint32_t *>(sh.cbuf + c0);
        } else {
            for (uint32_t c = c0 > shift ? c0 : shift; c < c0 + 4u && c < end; c++) dst[c - shift] = sh.cbuf[c];
        }
    }
}

#endif // BZH_GREP_CORE_H
