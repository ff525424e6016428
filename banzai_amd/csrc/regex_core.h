// regex_core.h -- THE THIRD MATCHER behind the tile front of search_core.h: the automaton of regex_plan.h, a DFA anchored at its
// start, walked from every start position as patset_core.h walks its trie -- the same class map, first-step row and dense table,
// with cycles in it.  Plain C++ without a launch in it: the kernels compile it for the device, tests/decode_host/regex_host.cpp for
// the host, where this very text runs thread by thread over a model of the LDS, under ASan and UBSan, against brute force.
// An automaton with assertions (^ $ \A \Z \b \B) takes THE LOOK-AROUND VARIANT at the end of this file (BzrLookMatcher;
// tests/decode_host/look_host.cpp); one without takes BzrMatcher, untouched.
//
// THE RULE, one for every caller: a hit is a start o at which some expression matches out[o .. o + L) for some 1 <= L <= max_span
// with o + L <= lim.  A start yields exactly ONE hit; len is the LONGEST such L, pattern the lowest-numbered expression that
// matches exactly that length.  A match longer than max_span is not found.
//
// THE WALK.  match16 and count16 stop at a start's first terminal: existence is all a grep and a count need (count16 is one per hit
// start).  Only emit1 walks on, to death or to its last step, and keeps the last terminal it passed.  Every bound of patset_core.h
// carries over: a walk takes at most min(max_len, lim - s) bytes, so it reads only staged text, and only entries below
// states * classes -- every state the table holds is below `states`, every class below `classes`.
//
// ROWS IN LDS.  A trie walk dies at its first step almost everywhere; a regex walk typically runs many ([a-z]+ walks every word to
// its end), and every step is a dependent load.  LDS_ROWS true: the table has at most BZR_LDS_ENTRIES entries and the workgroup
// stages all of it beside cls and first, so every step is an LDS read.  LDS_ROWS false: the table is read from HBM / L2 as a set's.
#ifndef BZH_REGEX_CORE_H
#define BZH_REGEX_CORE_H
#include "patset_core.h"

enum : uint32_t { BZR_LDS_ROWS = 2048 }; // = BZR_LDS_ENTRIES of regex_plan.h: 4 KiB, as much as the tile itself

struct BzrAuto { // the automaton, by value in the kernels' arguments: a set's fields, and the size of its table
    BzmSet m;
    uint32_t entries; // states * classes
};

template <bool LDS_ROWS>
struct BzrShared { // beside the tile
    __attribute__((aligned(4))) uint8_t cls[256];
    __attribute__((aligned(4))) uint16_t first[256];
    __attribute__((aligned(4))) uint16_t rows[LDS_ROWS ? (uint32_t)BZR_LDS_ROWS : 2u];
};

// Thread tid stages its part as bzm_stage does, and with LDS_ROWS its words of the table: entries [0, a.entries), pairs as words,
// an odd last one alone -- no read behind the table's last entry.  Returns its 16 bytes.  A barrier follows.
template <bool LDS_ROWS>
BZF_FN BzfVec bzr_stage(const uint8_t *d, uint64_t n, uint64_t t0, uint32_t tid, const BzrAuto &a, uint8_t *tile, BzrShared<LDS_ROWS> &sh)
{
    const BzmSet &m = a.m;
    if (tid < 64) reinterpret_cast<uint32_t *>(sh.cls)[tid] = reinterpret_cast<const uint32_t *>(m.cls)[tid];
    else if (tid < 192) reinterpret_cast<uint32_t *>(sh.first)[tid - 64] = reinterpret_cast<const uint32_t *>(m.first)[tid - 64];
    if (LDS_ROWS) {
        const uint32_t pairs = a.entries / 2; // (a.entries <= BZR_LDS_ROWS: the host chose this variant)
        for (uint32_t i = tid; i < pairs; i += BZF_THREADS) reinterpret_cast<uint32_t *>(sh.rows)[i] = reinterpret_cast<const uint32_t *>(m.table)[i];
        if ((a.entries & 1u) && tid == BZF_THREADS - 1) sh.rows[a.entries - 1] = m.table[a.entries - 1];
    }
    const BzfVec own = bzf_load16(d, n, t0 + tid * BZF_ITEMS);
    *reinterpret_cast<BzfVec *>(tile + tid * BZF_ITEMS) = own;
    if (tid * BZF_ITEMS < m.max_len - 1) *reinterpret_cast<BzfVec *>(tile + BZF_TILE + tid * BZF_ITEMS) = bzf_load16(d, n, t0 + BZF_TILE + tid * BZF_ITEMS);
    return own;
}

// The walk from one start (p < lim): text = the start's byte in the tile, st = its first transition, steps >= 1 the bytes it may
// take.  LONGEST false: returns the first terminal, *len its depth; true: the last one passed before death or step `steps`.
// Returns 0 where there is none.
template <bool LDS_ROWS, bool LONGEST>
BZF_FN uint32_t bzr_walk(const BzmSet &m, const BzrShared<LDS_ROWS> &sh, const uint8_t *text, uint32_t st, uint32_t steps, uint32_t *len)
{
    uint32_t depth = 1, best = 0;
    while (st) {
        if (st <= m.nterm) {
            best = st, *len = depth;
            if (!LONGEST) break;
        }
        if (depth >= steps) break;
        const uint32_t e = st * m.classes + sh.cls[text[depth]];
        st = LDS_ROWS ? sh.rows[e] : m.table[e];
        depth++;
    }
    return best;
}

// Behind the barrier: the starts among the thread's 16, of those in `valid`, at which some expression matches.
template <bool LDS_ROWS>
BZF_FN uint32_t bzr_match16(const BzfVec &own, uint32_t tid, uint64_t p0, const BzmSet &m, const uint8_t *tile, const BzrShared<LDS_ROWS> &sh, uint32_t valid)
{
    const uint8_t *mine = tile + tid * BZF_ITEMS;
    uint32_t hm = 0;
    for (uint32_t v = valid & bzf_range_mask16(p0, 0, m.lim); v; v &= v - 1u) { // (no start at or behind lim, whatever the caller says)
        const uint32_t k = (uint32_t)__builtin_ctz(v);
        const uint32_t st = sh.first[bzm_byte16(own, k)];
        uint32_t len;
        if (st && bzr_walk<LDS_ROWS, false>(m, sh, mine + k, st, bzm_steps(m, p0 + k), &len)) hm |= 1u << k;
    }
    return hm;
}

template <bool LDS_ROWS>
struct BzrMatcher { // the automaton as search_tiles and grep_tiles see it (patset_core.h: the matchers)
    using Shared = BzrShared<LDS_ROWS>;
    using Hit = BzmHit;
    static constexpr bool BY_LIM = true;
    BzrAuto a;
    BZF_MEM uint32_t delim() const { return a.m.delim; }
    BZF_MEM BzfVec stage(const uint8_t *d, uint64_t n, uint64_t t0, uint32_t tid, uint8_t *tile, Shared &sh) const { return bzr_stage<LDS_ROWS>(d, n, t0, tid, a, tile, sh); }
    BZF_MEM uint32_t match16(const BzfVec &own, uint32_t tid, uint64_t p0, const uint8_t *tile, const Shared &sh, uint32_t valid) const
    {
        return bzr_match16<LDS_ROWS>(own, tid, p0, a.m, tile, sh, valid);
    }
    BZF_MEM uint32_t count16(const BzfVec &own, uint32_t tid, uint64_t p0, const uint8_t *tile, const Shared &sh, uint32_t valid, uint32_t *hm) const
    {
        *hm = match16(own, tid, p0, tile, sh, valid);
        return (uint32_t)__builtin_popcount(*hm);
    }
    // the one hit of the start at tile byte `text` (position p; count16 found it live): the longest match
    BZF_MEM uint64_t emit1(const Shared &sh, const uint8_t *text, uint64_t p, uint64_t off, uint64_t rec, Hit *out, uint64_t rank, uint64_t emit) const
    {
        uint32_t len = 0;
        const uint32_t st = bzr_walk<LDS_ROWS, true>(a.m, sh, text, sh.first[text[0]], bzm_steps(a.m, p), &len);
        if (!st) return rank;
        if (rank < emit) out[rank] = BzmHit{off, rec, a.m.pat_no[st - 1], len};
        return rank + 1;
    }
};

// ---- THE LOOK-AROUND VARIANT: an automaton with assertions (^ $ \A \Z \b \B, the word and line wraps) -------------------------------
// An assertion sees ONE byte in front of its place and one behind it, each as a CONTEXT: the text's edge, 0x0A, a word byte, any
// other byte.  The compile resolves every assertion between two bytes inside the table; what is left to the walk are the two ends:
//   * THE START.  first[] has one row per distinct context in front of the start.  The byte in front of a start comes from the
//     thread's registers, for its first byte from the tile, for the tile's first byte from `prev`, one byte that thread 0 loads from
//     in front of the tile.  At position edge_lo no byte lies in front: the context there is ctx_lo, given by the window.
//   * THE END.  A terminal is a hit only if its mask holds the context of text[depth], the byte the walk reads next anyway.  At
//     position n that is the text's edge, never the zero bzf_load16 supplies: the windows let a walk reach n only where the whole
//     decoded text ends.
// The halo is one byte longer for it, max_len - 1 + look_ahead <= BZF_MAX_PATTERN: a match of 256 bytes from tile byte 4,095 looks
// ahead at the tile array's last byte.
enum : uint32_t { BZR_LOOK_EDGE = 0, BZR_LOOK_NL = 1, BZR_LOOK_WORD = 2, BZR_LOOK_OTHER = 3 };
BZF_FN uint32_t bzr_ctx(uint32_t b) // the context of a byte (regex_plan.h: bzr_ctx_of)
{
    if (b == 0x0Au) return BZR_LOOK_NL;
    const uint32_t l = b | 0x20u;
    return (l - 'a' < 26u) || (b - '0' < 10u) || b == '_' ? BZR_LOOK_WORD : BZR_LOOK_OTHER;
}

struct BzrLook { // beside BzrAuto, by value in the kernels' arguments
    const uint8_t *acc_mask; // [nterm] the contexts behind a match in which the terminal accepts, bit c
    const uint32_t *pat_ctx; // [nterm * 4] the lowest-numbered expression that accepts there
    uint32_t rows;           // start rows: first[rows * 256]
    uint32_t ctx_row;        // the start row of context c: bits [8 c, 8 c + 8)
    uint32_t look_ahead;     // 0: every mask holds every context, and no byte behind a match is read
    uint32_t ctx_lo;         // the context in front of position edge_lo, where no byte lies in front
    uint64_t edge_lo;
    uint64_t n;              // the text's end: behind it lies the text's edge
};

template <bool LDS_ROWS>
struct BzrLookShared { // beside the tile
    __attribute__((aligned(4))) uint8_t cls[256];
    __attribute__((aligned(4))) uint16_t first[4 * 256];
    __attribute__((aligned(4))) uint16_t rows[LDS_ROWS ? (uint32_t)BZR_LDS_ROWS : 2u];
    __attribute__((aligned(4))) uint8_t mask[LDS_ROWS ? (uint32_t)BZR_LDS_ROWS : 4u]; // (nterm < states <= entries)
    uint32_t prev; // the byte in front of the tile
};

static_assert((uint32_t)BZF_MAX_PATTERN - 1u + 1u <= (uint32_t)BZF_MAX_PATTERN, "the halo of a look-ahead, max_len - 1 + 1 bytes, lies inside the tile array");

template <bool LDS_ROWS>
BZF_FN BzfVec bzr_look_stage(const uint8_t *d, uint64_t n, uint64_t t0, uint32_t tid, const BzrAuto &a, const BzrLook &l, uint8_t *tile, BzrLookShared<LDS_ROWS> &sh)
{
    const BzmSet &m = a.m;
    if (tid < 64) reinterpret_cast<uint32_t *>(sh.cls)[tid] = reinterpret_cast<const uint32_t *>(m.cls)[tid];
    for (uint32_t i = tid; i < l.rows * 128u; i += BZF_THREADS) reinterpret_cast<uint32_t *>(sh.first)[i] = reinterpret_cast<const uint32_t *>(m.first)[i];
    if (LDS_ROWS) {
        const uint32_t pairs = a.entries / 2;
        for (uint32_t i = tid; i < pairs; i += BZF_THREADS) reinterpret_cast<uint32_t *>(sh.rows)[i] = reinterpret_cast<const uint32_t *>(m.table)[i];
        if ((a.entries & 1u) && tid == BZF_THREADS - 1) sh.rows[a.entries - 1] = m.table[a.entries - 1];
        for (uint32_t i = tid; i < m.nterm; i += BZF_THREADS) sh.mask[i] = l.acc_mask[i];
    }
    if (tid == 0) sh.prev = t0 > 0 ? d[t0 - 1] : 0u; // (t0 - 1 < n: a tile begins inside the text)
    const BzfVec own = bzf_load16(d, n, t0 + tid * BZF_ITEMS);
    *reinterpret_cast<BzfVec *>(tile + tid * BZF_ITEMS) = own;
    if (tid * BZF_ITEMS < m.max_len - 1 + l.look_ahead) *reinterpret_cast<BzfVec *>(tile + BZF_TILE + tid * BZF_ITEMS) = bzf_load16(d, n, t0 + BZF_TILE + tid * BZF_ITEMS);
    return own;
}

// the start row of position p, whose byte in front is `before` where one lies there
BZF_FN uint32_t bzr_look_row(const BzrLook &l, uint64_t p, uint32_t before)
{
    if (l.rows == 1) return 0;
    const uint32_t c = p == l.edge_lo ? l.ctx_lo : bzr_ctx(before);
    return (l.ctx_row >> (8 * c)) & 0xFFu;
}

// bzr_walk with the terminals judged by the context behind the match; to_end: the bytes between the start and the text's end.
// *ctx: the context behind the match that is returned
template <bool LDS_ROWS, bool LONGEST>
BZF_FN uint32_t bzr_look_walk(const BzmSet &m, const BzrLook &l, const BzrLookShared<LDS_ROWS> &sh, const uint8_t *text, uint32_t st, uint32_t steps, uint32_t to_end,
                              uint32_t *len, uint32_t *ctx)
{
    uint32_t depth = 1, best = 0;
    while (st) {
        if (st <= m.nterm) {
            const uint32_t c = !l.look_ahead ? 0u : depth == to_end ? (uint32_t)BZR_LOOK_EDGE : bzr_ctx(text[depth]);
            const uint32_t mask = LDS_ROWS ? sh.mask[st - 1] : l.acc_mask[st - 1];
            if (mask >> c & 1u) {
                best = st, *len = depth, *ctx = c;
                if (!LONGEST) break;
            }
        }
        if (depth >= steps) break;
        const uint32_t e = st * m.classes + sh.cls[text[depth]];
        st = LDS_ROWS ? sh.rows[e] : m.table[e];
        depth++;
    }
    return best;
}
BZF_FN uint32_t bzr_to_end(const BzrLook &l, uint64_t p) { return l.n - p < 0xFFFFu ? (uint32_t)(l.n - p) : 0xFFFFu; }

template <bool LDS_ROWS>
BZF_FN uint32_t bzr_look_match16(const BzfVec &own, uint32_t tid, uint64_t p0, const BzmSet &m, const BzrLook &l, const uint8_t *tile,
                                 const BzrLookShared<LDS_ROWS> &sh, uint32_t valid)
{
    const uint8_t *mine = tile + tid * BZF_ITEMS;
    uint32_t hm = 0;
    for (uint32_t v = valid & bzf_range_mask16(p0, 0, m.lim); v; v &= v - 1u) {
        const uint32_t k = (uint32_t)__builtin_ctz(v);
        const uint32_t before = k ? bzm_byte16(own, k - 1) : tid ? (uint32_t)mine[-1] : sh.prev;
        const uint32_t st = sh.first[bzr_look_row(l, p0 + k, before) * 256u + bzm_byte16(own, k)];
        uint32_t len, ctx;
        if (st && bzr_look_walk<LDS_ROWS, false>(m, l, sh, mine + k, st, bzm_steps(m, p0 + k), bzr_to_end(l, p0 + k), &len, &ctx)) hm |= 1u << k;
    }
    return hm;
}

template <bool LDS_ROWS>
struct BzrLookMatcher { // the automaton with assertions as search_tiles and grep_tiles see it
    using Shared = BzrLookShared<LDS_ROWS>;
    using Hit = BzmHit;
    static constexpr bool BY_LIM = true;
    BzrAuto a;
    BzrLook l;
    BZF_MEM uint32_t delim() const { return a.m.delim; }
    BZF_MEM BzfVec stage(const uint8_t *d, uint64_t n, uint64_t t0, uint32_t tid, uint8_t *tile, Shared &sh) const { return bzr_look_stage<LDS_ROWS>(d, n, t0, tid, a, l, tile, sh); }
    BZF_MEM uint32_t match16(const BzfVec &own, uint32_t tid, uint64_t p0, const uint8_t *tile, const Shared &sh, uint32_t valid) const
    {
        return bzr_look_match16<LDS_ROWS>(own, tid, p0, a.m, l, tile, sh, valid);
    }
    BZF_MEM uint32_t count16(const BzfVec &own, uint32_t tid, uint64_t p0, const uint8_t *tile, const Shared &sh, uint32_t valid, uint32_t *hm) const
    {
        *hm = match16(own, tid, p0, tile, sh, valid);
        return (uint32_t)__builtin_popcount(*hm);
    }
    // the one hit of the start at tile byte `text` (position p; count16 found it live): the longest match, and the expression that
    // accepts it behind its context.  The byte in front of a tile's first byte is sh.prev, of every other one its neighbour in the tile
    BZF_MEM uint64_t emit1(const Shared &sh, const uint8_t *text, uint64_t p, uint64_t off, uint64_t rec, Hit *out, uint64_t rank, uint64_t emit) const
    {
        uint32_t len = 0, ctx = 0;
        const uint32_t before = (p & (BZF_TILE - 1u)) ? (uint32_t)text[-1] : sh.prev;
        const uint32_t st = bzr_look_walk<LDS_ROWS, true>(a.m, l, sh, text, sh.first[bzr_look_row(l, p, before) * 256u + text[0]], bzm_steps(a.m, p), bzr_to_end(l, p), &len, &ctx);
        if (!st) return rank;
        if (rank < emit) out[rank] = BzmHit{off, rec, l.pat_ctx[(st - 1) * 4u + ctx], len};
        return rank + 1;
    }
};

#endif // BZH_REGEX_CORE_H
