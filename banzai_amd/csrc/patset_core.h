// patset_core.h -- THE SECOND MATCHER behind the tile front of search_core.h: a compiled set of byte strings (patset_plan.h),
// matched by a failureless trie walk from every start position, the way PFAC does it.  search_tiles and grep_tiles take a matcher
// as a template parameter; BzfOne below wraps the single pattern of search_core.h, BzmMatcher is the set.  Plain C++ without a
// launch in it: the kernels compile it for the device, tests/decode_host/patset_host.cpp for the host, where this very text runs
// thread by thread over a model of the LDS, under ASan and UBSan, against a naive matcher.
//
// THE RULE, one for every caller: pattern j of length L matches at start s iff the (folded) bytes agree and s + L <= lim, the end
// of the text or of the wanted range in the kernel's coordinates (lim <= n).
//
// THE WALK from a start: the first byte comes from the thread's registers, the first transition from first[256] in LDS (the
// root row behind the class map); every further byte from the tile and its halo of max_len - 1 bytes in LDS, its class from
// cls[256] in LDS, the transition by a plain load from the table in HBM.  A walk takes at most min(max_len, lim - s) bytes, so it
// reads no byte of the text that bzf_load16 did not stage, and no table entry outside [0, states * classes): every state the
// table holds is below `states`, every class below `classes`.  A walk passes at most one terminal per length, so a start yields at
// most min(distinct, 256) hits, in ascending length.
#ifndef BZH_PATSET_CORE_H
#define BZH_PATSET_CORE_H
#include "search_core.h"

#if defined(__HIPCC__)
#define BZF_MEM __host__ __device__ __forceinline__
#else
#define BZF_MEM inline
#endif

struct BzmSet { // the set, by value in the kernels' arguments; the pointers: HBM (the host's memory in the host harness)
    const uint8_t *cls;     // [256]
    const uint16_t *first;  // [256]
    const uint16_t *table;  // [states * classes]
    const uint32_t *pat_no; // [nterm]
    uint32_t classes, nterm, max_len, delim;
    uint64_t lim;           // of this window
};

struct BzmShared { // beside the tile
    __attribute__((aligned(4))) uint8_t cls[256];
    __attribute__((aligned(4))) uint16_t first[256];
};

// Thread tid of the tile at t0 stages its part: its 16 bytes and its share of the halo as bzf_stage does, its words of the class
// map and of the first transitions.  Returns its 16 bytes.  A barrier follows.
BZF_FN BzfVec bzm_stage(const uint8_t *d, uint64_t n, uint64_t t0, uint32_t tid, const BzmSet &m, uint8_t *tile, BzmShared &sh)
{
    if (tid < 64) reinterpret_cast<uint32_t *>(sh.cls)[tid] = reinterpret_cast<const uint32_t *>(m.cls)[tid];
    else if (tid < 192) reinterpret_cast<uint32_t *>(sh.first)[tid - 64] = reinterpret_cast<const uint32_t *>(m.first)[tid - 64];
    const BzfVec own = bzf_load16(d, n, t0 + tid * BZF_ITEMS);
    *reinterpret_cast<BzfVec *>(tile + tid * BZF_ITEMS) = own;
    if (tid * BZF_ITEMS < m.max_len - 1) *reinterpret_cast<BzfVec *>(tile + BZF_TILE + tid * BZF_ITEMS) = bzf_load16(d, n, t0 + BZF_TILE + tid * BZF_ITEMS);
    return own;
}

BZF_FN uint32_t bzm_byte16(const BzfVec &own, uint32_t k) // byte k of a thread's 16
{
    const uint32_t w = k < 8 ? (k < 4 ? own.x : own.y) : (k < 12 ? own.z : own.w);
    return (w >> (8 * (k & 3u))) & 0xFFu;
}
// the bytes a walk from position p may take
BZF_FN uint32_t bzm_steps(const BzmSet &m, uint64_t p) { return m.lim - p < m.max_len ? (uint32_t)(m.lim - p) : m.max_len; }

// The walk from one start (p < lim): text = the start's byte in the tile, st = its first transition.  Calls hit(state, length) at
// every terminal, shortest first, until hit returns false.
template <class F>
BZF_FN void bzm_walk(const BzmSet &m, const BzmShared &sh, const uint8_t *text, uint32_t st, uint32_t steps, F &&hit)
{
    uint32_t depth = 1;
    while (st) {
        if (st <= m.nterm && !hit(st, depth)) return;
        if (depth >= steps) return;
        st = m.table[(size_t)st * m.classes + sh.cls[text[depth]]];
        depth++;
    }
}

// the starts among the thread's 16, of those in `valid`, that a walk has to be made from: the first transition is alive
BZF_FN uint32_t bzm_alive16(const BzfVec &own, uint64_t p0, const BzmSet &m, const BzmShared &sh, uint32_t valid)
{
    uint32_t live = 0;
    for (uint32_t v = valid & bzf_range_mask16(p0, 0, m.lim); v; v &= v - 1u) { // (no start at or behind lim, whatever the caller says)
        const uint32_t k = (uint32_t)__builtin_ctz(v);
        if (sh.first[bzm_byte16(own, k)]) live |= 1u << k;
    }
    return live;
}

// Behind the barrier, for grep: the starts among the thread's 16, of those in `valid` (all of them in front of lim), at which
// at least one pattern matches.  A walk stops at its first terminal.
BZF_FN uint32_t bzm_match16(const BzfVec &own, uint32_t tid, uint64_t p0, const BzmSet &m, const uint8_t *tile, const BzmShared &sh, uint32_t valid)
{
    const uint8_t *mine = tile + tid * BZF_ITEMS;
    uint32_t hm = 0;
    for (uint32_t v = bzm_alive16(own, p0, m, sh, valid); v; v &= v - 1u) {
        const uint32_t k = (uint32_t)__builtin_ctz(v);
        bzm_walk(m, sh, mine + k, sh.first[mine[k]], bzm_steps(m, p0 + k), [&](uint32_t, uint32_t) { return hm |= 1u << k, false; });
    }
    return hm;
}

// For search: the (start, pattern) pairs among the thread's starts in `valid`; *hm = the starts that hold at least one.
BZF_FN uint32_t bzm_count16(const BzfVec &own, uint32_t tid, uint64_t p0, const BzmSet &m, const uint8_t *tile, const BzmShared &sh, uint32_t valid, uint32_t *hm)
{
    const uint8_t *mine = tile + tid * BZF_ITEMS;
    uint32_t c = 0, any = 0;
    for (uint32_t v = bzm_alive16(own, p0, m, sh, valid); v; v &= v - 1u) {
        const uint32_t k = (uint32_t)__builtin_ctz(v);
        bzm_walk(m, sh, mine + k, sh.first[mine[k]], bzm_steps(m, p0 + k), [&](uint32_t, uint32_t) { return c++, any |= 1u << k, true; });
    }
    *hm = any;
    return c;
}

struct BzmHit { // bzh_set_hit
    uint64_t off, record;
    uint32_t pattern, len;
};
// The pairs of one start at tile byte `text` (position p), in ascending length, into out[rank ..): those whose rank is below
// `emit` are stored.  Returns the rank behind them.
BZF_FN uint64_t bzm_emit1(const BzmSet &m, const BzmShared &sh, const uint8_t *text, uint64_t p, uint64_t off, uint64_t rec, BzmHit *out, uint64_t rank, uint64_t emit)
{
    bzm_walk(m, sh, text, sh.first[text[0]], bzm_steps(m, p), [&](uint32_t st, uint32_t len) {
        if (rank < emit) out[rank] = BzmHit{off, rec, m.pat_no[st - 1], len};
        rank++;
        return true;
    });
    return rank;
}

// ---- the matchers as search_tiles and grep_tiles see them ---------------------------------------------------------------------
// Shared: what the matcher keeps in LDS beside the tile.  stage: a thread's part of the staging, a barrier follows.  match16: the
// starts in `valid` that hold a match.  count16: the hits at those starts (*hm: the starts that hold one).  emit1: the hits of the
// start at tile byte `text` into the hit slots, the rank behind them returned.  longest1: the length of the longest match at a
// start that match16 named (match.hip: the matched parts alone), *pattern the lowest-numbered one of that length.  BY_LIM: the matcher bounds a match by lim itself,
// so every processed position is a start (a single pattern's starts end plen - 1 in front of the text's end instead).
struct BzfHit { // bzh_hit
    uint64_t off, record;
};
struct BzfOneShared {
    __attribute__((aligned(4))) uint8_t pat[BZF_MAX_PATTERN];
};
template <class M>
struct BzfOnePerStart { // count16 of a matcher M whose starts hold one hit each (the single pattern, an automaton): an empty base
    template <class S>
    BZF_MEM uint32_t count16(const BzfVec &own, uint32_t tid, uint64_t p0, const uint8_t *tile, const S &sh, uint32_t valid, uint32_t *hm) const
    {
        return (uint32_t)__builtin_popcount(*hm = static_cast<const M *>(this)->match16(own, tid, p0, tile, sh, valid));
    }
};
struct BzfOne : BzfOnePerStart<BzfOne> { // the single pattern of search_core.h
    using Shared = BzfOneShared;
    using Hit = BzfHit;
    static constexpr bool BY_LIM = false;
    BzfPattern p;
    BZF_MEM uint32_t delim() const { return p.delim; }
    BZF_MEM BzfVec stage(const uint8_t *d, uint64_t n, uint64_t t0, uint32_t tid, uint8_t *tile, Shared &sh) const { return bzf_stage(d, n, t0, tid, p, tile, sh.pat); }
    BZF_MEM uint32_t match16(const BzfVec &own, uint32_t tid, uint64_t, const uint8_t *tile, const Shared &sh, uint32_t valid) const { return bzf_match16(own, tid, p, tile, sh.pat, valid); }
    BZF_MEM uint64_t emit1(const Shared &, const uint8_t *, uint64_t, uint64_t off, uint64_t rec, Hit *out, uint64_t rank, uint64_t emit) const
    {
        if (rank < emit) out[rank] = Hit{off, rec};
        return rank + 1;
    }
    BZF_MEM uint32_t longest1(const Shared &, const uint8_t *, uint64_t, uint32_t *pattern) const { return *pattern = 0, p.plen; }
};
struct BzmMatcher { // the set
    using Shared = BzmShared;
    using Hit = BzmHit;
    static constexpr bool BY_LIM = true;
    BzmSet m;
    BZF_MEM uint32_t delim() const { return m.delim; }
    BZF_MEM BzfVec stage(const uint8_t *d, uint64_t n, uint64_t t0, uint32_t tid, uint8_t *tile, Shared &sh) const { return bzm_stage(d, n, t0, tid, m, tile, sh); }
    BZF_MEM uint32_t match16(const BzfVec &own, uint32_t tid, uint64_t p0, const uint8_t *tile, const Shared &sh, uint32_t valid) const
    {
        return bzm_match16(own, tid, p0, m, tile, sh, valid);
    }
    BZF_MEM uint32_t count16(const BzfVec &own, uint32_t tid, uint64_t p0, const uint8_t *tile, const Shared &sh, uint32_t valid, uint32_t *hm) const
    {
        return bzm_count16(own, tid, p0, m, tile, sh, valid, hm);
    }
    BZF_MEM uint64_t emit1(const Shared &sh, const uint8_t *text, uint64_t p, uint64_t off, uint64_t rec, Hit *out, uint64_t rank, uint64_t emit) const
    {
        return bzm_emit1(m, sh, text, p, off, rec, out, rank, emit);
    }
    BZF_MEM uint32_t longest1(const Shared &sh, const uint8_t *text, uint64_t p, uint32_t *pattern) const
    {
        uint32_t last = 0, best = 0; // (a walk's terminals ascend by length)
        bzm_walk(m, sh, text, sh.first[text[0]], bzm_steps(m, p), [&](uint32_t st, uint32_t len) { return last = st, best = len, true; });
        if (last) *pattern = m.pat_no[last - 1];
        return best;
    }
};

#endif // BZH_PATSET_CORE_H
