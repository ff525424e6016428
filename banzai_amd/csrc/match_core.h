// match_core.h -- what one thread, one tile and the two scans of match.hip do behind the tile front of search_core.h: the
// selection of the NON-OVERLAPPING, LEFTMOST-LONGEST matches (grep -o) and the compaction of their bytes.  Plain C++ of
// (tid, shared) without a launch in it: the kernels compile it for the device, tests/decode_host/match_host.cpp for the host, where
// this very text runs thread by thread and tile by tile over a model of the LDS, under ASan and UBSan, against a greedy loop.
//
// THE DEPENDENCY.  nxt(p) = p + L(p) at a processed start that holds a match (L: the matcher's longest1, 1..256), p + 1 elsewhere.
// The selected matches are the match starts on the orbit of the window's first byte under nxt (the window's starts are clipped to
// the cursor it was entered with: match_plan.h).  A tile of 4,096 positions is entered e bytes beyond its first byte, 0 <= e < 256,
// and left x bytes beyond the next tile's first byte: THE MAP of a tile, [0, 256) -> [0, 256).  Where some position of the tile is
// spanned by no match of an earlier start, every orbit passes it and the map is CONSTANT; `aa` in a run of `a` has no such position
// and its map is e -> e: such a tile is OPEN.
//
// INSIDE A TILE, three levels, no walk longer than 16 steps:
//   x[p]  the first position on p's orbit outside p's SEGMENT, the 16 positions of one thread: 16 steps down the segment, each
//         thread its own (mt_local);
//   y[p]  the first one outside p's GROUP of 256 positions: a step of x leaves a segment, a group has 16, so four rounds of
//         pointer doubling between two arrays (mt_group_step);
//   a match is at most 256 bytes, so an orbit enters EVERY group: 16 steps of y from an entry give the group entries and the exit
//         (mt_map: thread e for entry e; mt_group_entries: one thread for the true entry), 16 steps of x from a group's entry
//         the entered segments of the group (mt_seg_entries: one thread a group), 16 steps down a segment its selected starts
//         (mt_marks).
// ACROSS TILES: match_scan, one workgroup, every thread a chunk of consecutive tiles.  A chunk is composed for all 256 entries until
// it meets a constant tile, behind which one value is left; thread 0 chains the 256 chunks; every thread walks its chunk again
// with the true entry.  No thread follows the chain through more than its chunk.
//
// THE TABLES between the passes, all written by plain stores of the tile's own workgroup:
//   MtTile  [tiles]       the starts that hold a match, the delimiters, the map where it is constant; the scan adds the entry
//   map     [tiles * 256] the map of an open tile
//   hits    [tiles * 256] every thread's match starts, 16 bits
//   lens    [tiles * 4096] L - 1 at every match start, written and read only by threads that hold one
//   MtCount [tiles]       the selected matches, their bytes, where the last of them ends
//   MtBase  [tiles]       the delimiters (match_scan), the matches and bytes (match_sum) in front of every tile
#ifndef BZH_MATCH_CORE_H
#define BZH_MATCH_CORE_H
#include "patset_core.h"
#include "match_plan.h"

struct MtTile {
    uint32_t cand;  // starts that hold a match
    uint32_t nd;    // delimiters that count
    uint32_t konst; // bit 8: the map is constant, bits 0..7 its value
    uint32_t entry; // match_scan: where the tile is entered
};
struct MtCount {
    uint32_t cnt, bytes; // the selected matches that start in the tile, their bytes
    uint32_t last_end;   // where the last of them ends, from the tile's first byte (0: none)
    uint32_t pad;
};
struct MtBase {
    uint64_t cnt, bytes, del; // in front of the tile
};
struct MtEntry { // bzh_match_entry
    uint64_t off, record;
    uint32_t pattern, len;
    uint64_t out_off;
};
enum : uint32_t { MT_CONST = 0x100u, MT_GROUP = 256, MT_NONE = 0xFFFFu };

struct MtShared { // beside the tile and the matcher's tables
    uint16_t x[BZF_TILE];
    __attribute__((aligned(16))) uint16_t y[2][BZF_TILE]; // (the gather compacts the tile's bytes in it once the marks are made)
    uint16_t gent[BZF_TILE / MT_GROUP + 1]; // the entry of every group, and the exit
    uint16_t sent[BZF_THREADS];             // the entry of every segment (MT_NONE: the orbit skips it)
    uint8_t map[256];
    uint32_t any, open, last_end;
    uint64_t s[2][BZF_THREADS]; // the sums: matches | bytes << 16 | delimiters << 32
};
static_assert(sizeof(uint16_t) * 2 * BZF_TILE >= BZF_TILE + BZF_MAX_PATTERN, "the compacted bytes of a tile fit where y lay");

BZF_FN void mt_init(MtShared &sh, uint32_t tid)
{
    sh.sent[tid] = (uint16_t)MT_NONE;
    if (tid == 0) sh.any = 0, sh.open = 0, sh.last_end = 0;
}

// x of the thread's 16 positions.  hm: its match starts; len: L - 1 at each of them, byte k for position k
BZF_FN void mt_local(MtShared &sh, uint32_t tid, uint32_t hm, const BzfVec &len)
{
    uint16_t *x = sh.x + tid * BZF_ITEMS;
    for (uint32_t i = 0; i < BZF_ITEMS; i++) {
        const uint32_t o = BZF_ITEMS - 1 - i;
        const uint32_t nx = o + 1 + ((hm >> o & 1u) ? bzm_byte16(len, o) : 0u);
        x[o] = (uint16_t)(nx >= BZF_ITEMS ? tid * BZF_ITEMS + nx : x[nx]);
    }
}
// round r of 4: y of the thread's 16 positions, 2^(r + 1) steps of x or the first of them that leaves the group
BZF_FN void mt_group_step(MtShared &sh, uint32_t tid, uint32_t r)
{
    const uint16_t *src = r == 0 ? sh.x : sh.y[(r - 1) & 1u];
    uint16_t *dst = sh.y[r & 1u];
    for (uint32_t k = 0; k < BZF_ITEMS; k++) {
        const uint32_t p = tid * BZF_ITEMS + k, gend = (p | (MT_GROUP - 1u)) + 1u;
        uint32_t v = src[p];
        if (v < gend) v = src[v];
        dst[p] = (uint16_t)v;
    }
}
BZF_FN const uint16_t *mt_y(const MtShared &sh) { return sh.y[1]; } // (behind round 3)

// thread e: the exit of entry e
BZF_FN void mt_map(MtShared &sh, uint32_t tid)
{
    const uint16_t *y = mt_y(sh);
    uint32_t p = tid;
    for (uint32_t g = 0; g < BZF_TILE / MT_GROUP; g++) p = y[p];
    sh.map[tid] = (uint8_t)(p - BZF_TILE);
}
BZF_FN void mt_map_open(MtShared &sh, uint32_t tid)
{
    if (sh.map[tid] != sh.map[0]) sh.open = 1; // (every writer stores the same word)
}

// one thread: the groups' entries from the tile's
BZF_FN void mt_group_entries(MtShared &sh, uint32_t entry)
{
    const uint16_t *y = mt_y(sh);
    uint32_t p = entry;
    for (uint32_t g = 0; g < BZF_TILE / MT_GROUP; g++) sh.gent[g] = (uint16_t)p, p = y[p];
    sh.gent[BZF_TILE / MT_GROUP] = (uint16_t)p;
}
// thread g < 16: the entered segments of group g
BZF_FN void mt_seg_entries(MtShared &sh, uint32_t g)
{
    const uint32_t gend = (g + 1u) * MT_GROUP;
    for (uint32_t p = sh.gent[g]; p < gend; p = sh.x[p]) sh.sent[p / BZF_ITEMS] = (uint16_t)p;
}
// L - 1 at position o of a thread's 16, o not known at compile time: two selects and a shift, no table
BZF_FN uint32_t mt_len16(const BzfVec &len, uint32_t o)
{
    const uint64_t lo = len.x | (uint64_t)len.y << 32, hi = len.z | (uint64_t)len.w << 32;
    return (uint32_t)((o < 8 ? lo : hi) >> (8u * (o & 7u))) & 0xFFu;
}
// the thread's selected starts, their bytes, and where the last of them ends
BZF_FN uint32_t mt_marks(const MtShared &sh, uint32_t tid, uint32_t hm, const BzfVec &len, uint32_t *bytes, uint32_t *last_end)
{
    uint32_t sm = 0, b = 0, e = 0;
    const uint32_t p = sh.sent[tid];
    if (p != MT_NONE) {
        uint32_t o = p - tid * BZF_ITEMS;
        while (o < BZF_ITEMS) {
            if (hm >> o & 1u) {
                const uint32_t l = mt_len16(len, o) + 1u;
                sm |= 1u << o, b += l, e = tid * BZF_ITEMS + o + l;
                o += l;
            } else {
                o++;
            }
        }
    }
    *bytes = b, *last_end = e;
    return sm;
}

// the sums over the workgroup: 8 rounds, s[0] holds the inclusive ones behind them
BZF_FN void mt_sum_put(MtShared &sh, uint32_t tid, uint32_t cnt, uint32_t bytes, uint32_t nd) { sh.s[0][tid] = cnt | (uint64_t)bytes << 16 | (uint64_t)nd << 32; }
BZF_FN void mt_sum_step(MtShared &sh, uint32_t tid, uint32_t k)
{
    const uint64_t *src = sh.s[k & 1u];
    sh.s[(k + 1u) & 1u][tid] = src[tid] + (tid >= (1u << k) ? src[tid - (1u << k)] : 0u);
}
BZF_FN uint64_t mt_sum_excl(const MtShared &sh, uint32_t tid) { return tid ? sh.s[0][tid - 1] : 0u; }
BZF_FN uint64_t mt_sum_all(const MtShared &sh) { return sh.s[0][BZF_THREADS - 1]; }
BZF_FN uint32_t mt_s_cnt(uint64_t v) { return (uint32_t)v & 0xFFFFu; }
BZF_FN uint32_t mt_s_bytes(uint64_t v) { return (uint32_t)(v >> 16) & 0xFFFFu; }
BZF_FN uint32_t mt_s_del(uint64_t v) { return (uint32_t)(v >> 32); }

// the thread that holds the tile's last selected start says where it ends (behind the sums of the counts)
BZF_FN void mt_last_end(MtShared &sh, uint32_t tid, uint32_t sm, uint32_t last_end)
{
    if (sm && mt_s_cnt(sh.s[0][tid]) == mt_s_cnt(mt_sum_all(sh))) sh.last_end = last_end;
}

// The gather of one thread: an entry for every selected start and its bytes from the tile and its halo into comp, the tile's
// compacted bytes.  s0: the sums in front of the thread; dm: its delimiter bits; mine: its first byte in the tile.  `longest`
// gives the pattern number of a start.  Stores entries of this tile only, at their ranks in the window.
template <class M>
BZF_FN void mt_gather(const M &m, const typename M::Shared &msh, uint8_t *comp, uint32_t sm, const BzfVec &len, uint32_t dm, uint64_t s0, const uint8_t *mine,
                      uint64_t p0, const BzfWindow &w, uint32_t records, const MtBase &base, uint64_t out_base, bool want_out, MtEntry *ent)
{
    uint64_t rank = base.cnt + mt_s_cnt(s0);
    uint32_t at = mt_s_bytes(s0);
    for (; sm; sm &= sm - 1u) {
        const uint32_t k = (uint32_t)__builtin_ctz(sm), l = mt_len16(len, k) + 1u;
        const uint64_t pos = p0 + k;
        if (ent) {
            uint64_t rec = 0;
            if (records) {
                if (pos >= w.d_lo) {
                    rec = w.rec_base + base.del + mt_s_del(s0) + bzf_delims_before(dm, k);
                } else { // a start in the carry: the delimiters between it and d_lo were counted by the window before
                    const uint32_t gap = w.d_lo - pos < (uint64_t)BZF_MAX_PATTERN ? (uint32_t)(w.d_lo - pos) : (uint32_t)BZF_MAX_PATTERN; // (the halo holds them)
                    uint32_t c = 0;
                    for (uint32_t j = 0; j < gap; j++) c += mine[k + j] == m.delim();
                    rec = w.rec_base - c;
                }
            }
            uint32_t pattern = 0;
            (void)m.longest1(msh, mine + k, pos, &pattern);
            ent[rank] = MtEntry{w.off_base + pos, rec, pattern, l, out_base + base.bytes + at};
        }
        if (want_out)
            for (uint32_t j = 0; j < l; j++) comp[at + j] = mine[k + j];
        rank++, at += l;
    }
}
// comp[0, bytes) to dst: single bytes up to the first aligned word and behind the last, words between them
BZF_FN void mt_store(const uint8_t *comp, uint32_t tid, uint8_t *dst, uint32_t bytes)
{
    uint32_t head = (4u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u;
    if (head > bytes) head = bytes;
    const uint32_t words = (bytes - head) / 4u, tail = bytes - head - 4u * words;
    if (tid < head) dst[tid] = comp[tid];
    for (uint32_t j = tid; j < words; j += BZF_THREADS) {
        const uint8_t *c = comp + head + 4u * j;
        *reinterpret_cast<uint32_t *>(dst + head + 4u * j) = (uint32_t)c[0] | (uint32_t)c[1] << 8 | (uint32_t)c[2] << 16 | (uint32_t)c[3] << 24;
    }
    if (tid < tail) dst[head + 4u * words + tid] = comp[head + 4u * words + tid];
}

// ---- match_scan: the entry of every tile ----------------------------------------------------------------------------------------
enum : uint32_t { MT_CHUNK_IDENT = 0, MT_CHUNK_CONST = 1, MT_CHUNK_TABLE = 2 };
struct MtScanShared {
    uint8_t kind[BZF_THREADS], val[BZF_THREADS], in[BZF_THREADS];
    uint64_t del[BZF_THREADS];
    uint32_t cand[BZF_THREADS], open[BZF_THREADS], entered[BZF_THREADS];
};
BZF_FN void mt_chunk(uint32_t tid, uint32_t tiles, uint32_t *lo, uint32_t *hi)
{
    const uint32_t c = (tiles + BZF_THREADS - 1) / BZF_THREADS;
    *lo = tiles < tid * c ? tiles : tid * c;
    *hi = tiles < *lo + c ? tiles : *lo + c;
}
BZF_FN uint32_t mt_apply(const MtTile &x, const uint8_t *map, uint32_t t, uint32_t e) { return (x.konst & MT_CONST) ? (x.konst & 0xFFu) : map[(size_t)t * 256u + e]; }
// the thread's chunk composed: one value from its first constant tile on, all 256 in its row of summ [256 * 256] in front of one
BZF_FN void mt_scan_a(MtScanShared &sh, uint32_t tid, const MtTile *tile, const uint8_t *map, uint32_t tiles, uint8_t *summ)
{
    uint32_t lo, hi, kind = MT_CHUNK_IDENT, val = 0, cand = 0, open = 0;
    uint64_t del = 0;
    uint8_t *row = summ + (size_t)tid * 256u;
    mt_chunk(tid, tiles, &lo, &hi);
    for (uint32_t t = lo; t < hi; t++) {
        const MtTile x = tile[t];
        cand += x.cand, del += x.nd, open += !(x.konst & MT_CONST);
        if (x.konst & MT_CONST) kind = MT_CHUNK_CONST, val = x.konst & 0xFFu;
        else if (kind == MT_CHUNK_CONST) val = map[(size_t)t * 256u + val];
        else
            for (uint32_t e = 0; e < 256; e++) row[e] = map[(size_t)t * 256u + (kind == MT_CHUNK_IDENT ? e : row[e])];
        if (kind == MT_CHUNK_IDENT) kind = MT_CHUNK_TABLE; // (an open first tile)
    }
    sh.kind[tid] = (uint8_t)kind, sh.val[tid] = (uint8_t)val;
    sh.cand[tid] = cand, sh.open[tid] = open, sh.del[tid] = del;
}
// one thread: the chain of the chunks from the window's entry, 0; the delimiters in front of every chunk
BZF_FN void mt_scan_b(MtScanShared &sh, const uint8_t *summ, uint64_t *totals)
{
    uint32_t e = 0;
    uint64_t del = 0, cand = 0, open = 0;
    for (uint32_t k = 0; k < BZF_THREADS; k++) {
        sh.in[k] = (uint8_t)e;
        if (sh.kind[k] == MT_CHUNK_CONST) e = sh.val[k];
        else if (sh.kind[k] == MT_CHUNK_TABLE) e = summ[(size_t)k * 256u + e];
        const uint64_t d = sh.del[k];
        sh.del[k] = del, del += d;
        cand += sh.cand[k], open += sh.open[k];
    }
    totals[MT_T_DEL] = del, totals[MT_T_CAND] = cand, totals[MT_T_OPEN] = open;
}
// the chunk again with its true entry
BZF_FN void mt_scan_c(MtScanShared &sh, uint32_t tid, MtTile *tile, const uint8_t *map, uint32_t tiles, MtBase *base)
{
    uint32_t lo, hi, e = sh.in[tid], entered = 0;
    uint64_t del = sh.del[tid];
    mt_chunk(tid, tiles, &lo, &hi);
    for (uint32_t t = lo; t < hi; t++) {
        const MtTile x = tile[t];
        tile[t].entry = e, base[t].del = del;
        entered += e != 0, del += x.nd;
        e = mt_apply(x, map, t, e);
    }
    sh.entered[tid] = entered;
}
BZF_FN void mt_scan_d(const MtScanShared &sh, uint64_t *totals)
{
    uint64_t entered = 0;
    for (uint32_t k = 0; k < BZF_THREADS; k++) entered += sh.entered[k];
    totals[MT_T_ENTERED] = entered;
}

// ---- match_sum: the matches and bytes in front of every tile ----------------------------------------------------------------------
struct MtSumShared {
    uint64_t cnt[BZF_THREADS], bytes[BZF_THREADS], cursor[BZF_THREADS];
};
BZF_FN void mt_sum_a(MtSumShared &sh, uint32_t tid, const MtCount *cnt, uint32_t tiles)
{
    uint32_t lo, hi;
    uint64_t c = 0, b = 0, cur = 0;
    mt_chunk(tid, tiles, &lo, &hi);
    for (uint32_t t = lo; t < hi; t++) {
        const MtCount x = cnt[t];
        c += x.cnt, b += x.bytes;
        if (x.cnt) cur = (uint64_t)t * BZF_TILE + x.last_end;
    }
    sh.cnt[tid] = c, sh.bytes[tid] = b, sh.cursor[tid] = cur;
}
BZF_FN void mt_sum_b(MtSumShared &sh, uint64_t *totals)
{
    uint64_t c = 0, b = 0, cur = 0;
    for (uint32_t k = 0; k < BZF_THREADS; k++) {
        const uint64_t vc = sh.cnt[k], vb = sh.bytes[k];
        if (vc) cur = sh.cursor[k];
        sh.cnt[k] = c, sh.bytes[k] = b;
        c += vc, b += vb;
    }
    totals[MT_T_SEL] = c, totals[MT_T_BYTES] = b, totals[MT_T_CURSOR] = cur;
}
BZF_FN void mt_sum_c(const MtSumShared &sh, uint32_t tid, const MtCount *cnt, uint32_t tiles, MtBase *base)
{
    uint32_t lo, hi;
    uint64_t c = sh.cnt[tid], b = sh.bytes[tid];
    mt_chunk(tid, tiles, &lo, &hi);
    for (uint32_t t = lo; t < hi; t++) {
        base[t].cnt = c, base[t].bytes = b;
        c += cnt[t].cnt, b += cnt[t].bytes;
    }
}

#endif // BZH_MATCH_CORE_H
