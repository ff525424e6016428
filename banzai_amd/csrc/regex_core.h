// regex_core.h -- THE THIRD MATCHER behind the tile front of search_core.h: the automaton of regex_plan.h, a DFA anchored at its
// start, walked from every start position as patset_core.h walks its trie -- the same class map, first-step row and dense table,
// with cycles in it.  Plain C++ without a launch in it: the kernels compile it for the device, tests/decode_host/regex_host.cpp and
// look_host.cpp for the host, where this very text runs thread by thread over a model of the LDS, under ASan and UBSan, against
// brute force.  ONE matcher, BzrMatcher<LDS_ROWS, LOOK>: an automaton with assertions (^ $ \A \Z \b \B) takes LOOK true, one
// without takes LOOK false, which holds nothing of the other's -- no BzrLook in its kernel argument, no byte of LDS more.
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
//
// LOOK: an assertion sees ONE byte in front of its place and one behind it, each as a CONTEXT: the text's edge, 0x0A, a word byte,
// any other byte.  The compile resolves every assertion between two bytes inside the table; what is left to the walk are the two ends:
//   * THE START.  first[] has one row per distinct context in front of the start.  The byte in front of a start comes from the
//     thread's registers, for its first byte from the tile, for the tile's first byte from `prev`, one byte that thread 0 loads from
//     in front of the tile.  At position edge_lo no byte lies in front: the context there is ctx_lo, given by the window.
//   * THE END.  A terminal is a hit only if its mask holds the context of text[depth], the byte the walk reads next anyway.  At
//     position n that is the text's edge, never the zero bzf_load16 supplies: the windows let a walk reach n only where the whole
//     decoded text ends.
// The halo is one byte longer for it, max_len - 1 + look_ahead <= BZF_MAX_PATTERN: a match of 256 bytes from tile byte 4,095 looks
// ahead at the tile array's last byte.
#ifndef BZH_REGEX_CORE_H
#define BZH_REGEX_CORE_H
#include "patset_core.h"

enum : uint32_t { BZR_LDS_ROWS = 2048 }; // = BZR_LDS_ENTRIES of regex_plan.h: 4 KiB, as much as the tile itself

struct BzrAuto { // the automaton, by value in the kernels' arguments: a set's fields, and the size of its table
    BzmSet m;
    uint32_t entries; // states * classes
};

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
// the start row of position p, whose byte in front is `before` where one lies there
BZF_FN uint32_t bzr_look_row(const BzrLook &l, uint64_t p, uint32_t before)
{
    if (l.rows == 1) return 0;
    const uint32_t c = p == l.edge_lo ? l.ctx_lo : bzr_ctx(before);
    return (l.ctx_row >> (8 * c)) & 0xFFu;
}
BZF_FN uint32_t bzr_to_end(const BzrLook &l, uint64_t p) { return l.n - p < 0xFFFFu ? (uint32_t)(l.n - p) : 0xFFFFu; } // the bytes between a start and the text's end

template <bool LOOK>
struct BzrArgs { // what a matcher holds in the kernels' arguments ...
    BzrAuto a;
};
template <>
struct BzrArgs<true> { // ... and with assertions
    BzrAuto a;
    BzrLook l;
};

template <bool LDS_ROWS, bool LOOK>
struct BzrTables { // beside the tile
    __attribute__((aligned(4))) uint8_t cls[256];
    __attribute__((aligned(4))) uint16_t first[LOOK ? 4 * 256 : 256];
    __attribute__((aligned(4))) uint16_t rows[LDS_ROWS ? (uint32_t)BZR_LDS_ROWS : 2u];
};
template <bool LDS_ROWS, bool LOOK>
struct BzrLookLds {}; // ... behind them nothing without assertions, ...
template <bool LDS_ROWS>
struct BzrLookLds<LDS_ROWS, true> { // ... with them the terminals' masks and one byte
    __attribute__((aligned(4))) uint8_t mask[LDS_ROWS ? (uint32_t)BZR_LDS_ROWS : 4u]; // (nterm < states <= entries)
    uint32_t prev; // the byte in front of the tile
};
template <bool LDS_ROWS, bool LOOK>
struct BzrShared : BzrTables<LDS_ROWS, LOOK>, BzrLookLds<LDS_ROWS, LOOK> {};

static_assert(sizeof(BzrShared<false, false>) == 256 + 512 + 4 && sizeof(BzrShared<true, false>) == 256 + 512 + 2 * BZR_LDS_ROWS, "without assertions: cls, first, rows");
static_assert((uint32_t)BZF_MAX_PATTERN - 1u + 1u <= (uint32_t)BZF_MAX_PATTERN, "the halo of a look-ahead, max_len - 1 + 1 bytes, lies inside the tile array");

// The automaton as search_tiles and grep_tiles see it (patset_core.h: the matchers).  The arguments are its first base, so
// BzrMatcher<L>{BzrAuto{..}} still names and makes the matcher without assertions, as it did when that was a type of its own.
template <bool LDS_ROWS, bool LOOK = false>
struct BzrMatcher : BzrArgs<LOOK>, BzfOnePerStart<BzrMatcher<LDS_ROWS, LOOK>> {
    using Shared = BzrShared<LDS_ROWS, LOOK>;
    using Hit = BzmHit;
    static constexpr bool BY_LIM = true;
    BZF_MEM uint32_t delim() const { return this->a.m.delim; }
    // Thread tid stages its part as bzm_stage does -- with assertions every start row, the byte in front of the tile and a halo
    // one byte longer -- and with LDS_ROWS its words of the table: entries [0, a.entries), pairs as words, an odd last one alone
    // -- no read behind the table's last entry -- and the masks.  Returns its 16 bytes.  A barrier follows.
    BZF_MEM BzfVec stage(const uint8_t *d, uint64_t n, uint64_t t0, uint32_t tid, uint8_t *tile, Shared &sh) const
    {
        const BzrAuto &a = this->a;
        const BzmSet &m = a.m;
        uint32_t halo = m.max_len - 1;
        if (tid < 64) reinterpret_cast<uint32_t *>(sh.cls)[tid] = reinterpret_cast<const uint32_t *>(m.cls)[tid];
        else if (!LOOK && tid < 192) reinterpret_cast<uint32_t *>(sh.first)[tid - 64] = reinterpret_cast<const uint32_t *>(m.first)[tid - 64];
        if constexpr (LOOK)
            for (uint32_t i = tid; i < this->l.rows * 128u; i += BZF_THREADS) reinterpret_cast<uint32_t *>(sh.first)[i] = reinterpret_cast<const uint32_t *>(m.first)[i];
        if (LDS_ROWS) {
            const uint32_t pairs = a.entries / 2; // (a.entries <= BZR_LDS_ROWS: the host chose this variant)
            for (uint32_t i = tid; i < pairs; i += BZF_THREADS) reinterpret_cast<uint32_t *>(sh.rows)[i] = reinterpret_cast<const uint32_t *>(m.table)[i];
            if ((a.entries & 1u) && tid == BZF_THREADS - 1) sh.rows[a.entries - 1] = m.table[a.entries - 1];
            if constexpr (LOOK)
                for (uint32_t i = tid; i < m.nterm; i += BZF_THREADS) sh.mask[i] = this->l.acc_mask[i];
        }
        if constexpr (LOOK) {
            if (tid == 0) sh.prev = t0 > 0 ? d[t0 - 1] : 0u; // (t0 - 1 < n: a tile begins inside the text)
            halo += this->l.look_ahead;
        }
        const BzfVec own = bzf_load16(d, n, t0 + tid * BZF_ITEMS);
        *reinterpret_cast<BzfVec *>(tile + tid * BZF_ITEMS) = own;
        if (tid * BZF_ITEMS < halo) *reinterpret_cast<BzfVec *>(tile + BZF_TILE + tid * BZF_ITEMS) = bzf_load16(d, n, t0 + BZF_TILE + tid * BZF_ITEMS);
        return own;
    }
    // where in sh.first the start row of position p begins; before: the byte in front of it where one lies there
    BZF_MEM uint32_t row(uint64_t p, uint32_t before) const
    {
        if constexpr (LOOK) return bzr_look_row(this->l, p, before) * 256u;
        else return 0;
    }
    // The walk from the start at position p < lim: text = the start's byte in the tile, st = its first transition; it takes at most
    // bzm_steps bytes.  LONGEST false: returns the first terminal, *len its depth; true: the last one passed before death or the
    // last step.  Returns 0 where there is none.  With assertions a terminal counts where its mask holds the context behind the
    // match, *ctx that of the one returned.
    template <bool LONGEST>
    BZF_MEM uint32_t walk(const Shared &sh, const uint8_t *text, uint32_t st, uint64_t p, uint32_t *len, uint32_t *ctx) const
    {
        const BzmSet &m = this->a.m;
        const uint32_t steps = bzm_steps(m, p);
        uint32_t to_end = 0;
        if constexpr (LOOK) to_end = bzr_to_end(this->l, p);
        uint32_t depth = 1, best = 0;
        while (st) {
            if (st <= m.nterm) {
                uint32_t c = 0;
                bool accepts = true;
                if constexpr (LOOK) {
                    c = !this->l.look_ahead ? 0u : depth == to_end ? (uint32_t)BZR_LOOK_EDGE : bzr_ctx(text[depth]);
                    const uint32_t mask = LDS_ROWS ? sh.mask[st - 1] : this->l.acc_mask[st - 1];
                    accepts = mask >> c & 1u;
                }
                if (accepts) {
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
    // Behind the barrier: the starts among the thread's 16, of those in `valid`, at which some expression matches.
    BZF_MEM uint32_t match16(const BzfVec &own, uint32_t tid, uint64_t p0, const uint8_t *tile, const Shared &sh, uint32_t valid) const
    {
        const uint8_t *mine = tile + tid * BZF_ITEMS;
        uint32_t hm = 0;
        for (uint32_t v = valid & bzf_range_mask16(p0, 0, this->a.m.lim); v; v &= v - 1u) { // (no start at or behind lim, whatever the caller says)
            const uint32_t k = (uint32_t)__builtin_ctz(v);
            uint32_t before = 0;
            if constexpr (LOOK) before = k ? bzm_byte16(own, k - 1) : tid ? (uint32_t)mine[-1] : sh.prev;
            const uint32_t st = sh.first[row(p0 + k, before) + bzm_byte16(own, k)];
            uint32_t len, ctx;
            if (st && walk<false>(sh, mine + k, st, p0 + k, &len, &ctx)) hm |= 1u << k;
        }
        return hm;
    }
    // the one hit of the start at tile byte `text` (position p; count16 found it live): the longest match, and with assertions the
    // expression that accepts it behind its context.  The byte in front of a tile's first byte is sh.prev, of every other one its
    // neighbour in the tile
    BZF_MEM uint64_t emit1(const Shared &sh, const uint8_t *text, uint64_t p, uint64_t off, uint64_t rec, Hit *out, uint64_t rank, uint64_t emit) const
    {
        uint32_t len = 0, ctx = 0, before = 0;
        if constexpr (LOOK) before = (p & (BZF_TILE - 1u)) ? (uint32_t)text[-1] : sh.prev;
        const uint32_t st = walk<true>(sh, text, sh.first[row(p, before) + text[0]], p, &len, &ctx);
        if (!st) return rank;
        if (rank < emit) out[rank] = BzmHit{off, rec, pattern(st, ctx), len};
        return rank + 1;
    }
    // the length of that hit alone, *pattern its expression (0: no match at this start)
    BZF_MEM uint32_t longest1(const Shared &sh, const uint8_t *text, uint64_t p, uint32_t *pat) const
    {
        uint32_t len = 0, ctx = 0, before = 0;
        if constexpr (LOOK) before = (p & (BZF_TILE - 1u)) ? (uint32_t)text[-1] : sh.prev;
        const uint32_t st = walk<true>(sh, text, sh.first[row(p, before) + text[0]], p, &len, &ctx);
        if (!st) return 0;
        *pat = pattern(st, ctx);
        return len;
    }
    BZF_MEM uint32_t pattern(uint32_t st, uint32_t ctx) const // the lowest-numbered expression that accepts at terminal st (behind context ctx)
    {
        if constexpr (LOOK) return this->l.pat_ctx[(st - 1) * 4u + ctx];
        else return this->a.m.pat_no[st - 1];
    }
};

#endif // BZH_REGEX_CORE_H
