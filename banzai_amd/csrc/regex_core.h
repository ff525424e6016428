// regex_core.h -- THE THIRD MATCHER behind the tile front of search_core.h: the automaton of regex_plan.h, a DFA anchored at its
// start, walked from every start position as patset_core.h walks its trie -- the same class map, first-step row and dense table,
// with cycles in it.  Plain C++ without a launch in it: the kernels compile it for the device, tests/decode_host/regex_host.cpp for
// the host, where this very text runs thread by thread over a model of the LDS, under ASan and UBSan, against brute force.
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

#endif // BZH_REGEX_CORE_H
