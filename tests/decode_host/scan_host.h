// scan_host.h -- ONE model of the two kernels of banzai_amd/csrc/search.hip and grep.hip and of the host code round them, shared by
// search_host, grep_host, patset_host, regex_host and look_host.  It is templated on the matcher M, so what runs thread by thread
// over the model LDS is the matcher interface of patset_core.h -- stage, match16, count16, emit1, the kernels' own text -- as
// search_tiles and grep_tiles run it: Group<M> is the workgroup, search_front / search_run are search_tiles' two passes and
// search_scan, grep_front / grep_run are grep_tiles' two passes and grep_scan with grep_core.h's phases, grep_call is GrepSink with
// its windows, its staging, GrepSink::finish and the tail.  A transcription of the kernels and nothing more: no truth, no case is here.
// The including program defines HOST_NAME, its name in a failing check's text, first.
#ifndef BZH_SCAN_HOST_H
#define BZH_SCAN_HOST_H
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "../../banzai_amd/csrc/grep_core.h"
#include "../../banzai_amd/csrc/grep_plan.h"
#include "../../banzai_amd/csrc/patset_core.h"
#include "../../banzai_amd/csrc/search_plan.h"
#include "tile_host.h"

static uint64_t rng_state;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}
static uint64_t below(uint64_t n) { return n ? rnd() % n : 0; }

#define CHECK(cond, ...)                                 \
    do {                                                 \
        if (!(cond)) {                                   \
            fprintf(stderr, HOST_NAME ": %s: ", #cond);  \
            fprintf(stderr, __VA_ARGS__);                \
            fprintf(stderr, "\n");                       \
            exit(1);                                     \
        }                                                \
    } while (0)
#define EVERY for (uint32_t tid = 0; tid < BZF_THREADS; tid++)
typedef std::vector<uint8_t> Bytes;
typedef unsigned long long ull;

template <class T>
static T *exact(const T *src, size_t count) // a copy in an allocation of exactly its size (count 0: one byte nobody may touch)
{
    T *p = (T *)malloc(count ? count * sizeof(T) : 1);
    if (!p) abort();
    if (count) memcpy(p, src, count * sizeof(T));
    return p;
}

// What no thread stores is not known: the tile array before staging, and the front of a staging buffer that no carry covers.  (A
// program whose matcher looks at a neighbour byte sets both to a word byte, so that a look at one of them shows.)
static uint8_t poison_tile = 0xAA, poison_front = 0xCC;

template <class M>
constexpr bool ONE_PER_START = std::is_base_of<BzfOnePerStart<M>, M>::value; // a start holds one hit (patset_core.h)

// ---- one workgroup: its LDS at the kernels' exact sizes and its threads' registers ------------------------------------------------
template <class M>
struct Group {
    uint8_t *tile;
    typename M::Shared *msh;
    BzgShared *sh;
    BzfVec own[BZF_THREADS];
    uint32_t hm[BZF_THREADS], nh[BZF_THREADS], dm[BZF_THREADS];
    BzgThread th[BZF_THREADS];
    Group() : msh(new typename M::Shared), sh(new BzgShared)
    {
        if (posix_memalign((void **)&tile, 16, BZF_TILE + BZF_MAX_PATTERN)) abort();
    }
    ~Group() { free(tile), delete msh, delete sh; }
    Group(const Group &) = delete;
    void stage(const M &m, const uint8_t *d, uint64_t n, uint64_t t) // tile t of d[0, n): M::stage in every thread, up to the barrier
    {
        memset(tile, poison_tile, BZF_TILE + BZF_MAX_PATTERN), memset((void *)msh, 0xAA, sizeof *msh), memset((void *)sh, 0xAA, sizeof *sh);
        EVERY own[tid] = m.stage(d, n, t * BZF_TILE, tid, tile, *msh);
    }
};

// ---- search_tiles up to the counts of every thread --------------------------------------------------------------------------------
template <class M>
static void search_front(const uint8_t *d, const BzfWindow &w, const M &m, bool records, uint64_t t, Group<M> &g)
{
    g.stage(m, d, w.n, t);
    EVERY {
        const uint64_t p0 = t * BZF_TILE + tid * BZF_ITEMS;
        const BzfVec &v = g.own[tid];
        const uint32_t valid = bzf_range_mask16(p0, w.s_lo, w.s_hi);
        g.nh[tid] = m.count16(v, tid, p0, g.tile, *g.msh, valid, &g.hm[tid]);
        CHECK(g.hm[tid] == m.match16(v, tid, p0, g.tile, *g.msh, valid) && (!ONE_PER_START<M> || g.nh[tid] == (uint32_t)__builtin_popcount(g.hm[tid])),
              "count16 and match16 name the same starts, one hit each where the matcher says so");
        g.dm[tid] = records ? bzf_eq_mask16(v.x, v.y, v.z, v.w, m.delim()) & bzf_range_mask16(p0, w.d_lo, w.n) : 0u;
    }
}
// search_window_run: both passes and search_scan between them.  out: the window's hit slots, exactly w.emit of them
template <class M>
static void search_run(const uint8_t *d, BzfWindow w, const M &m, bool records, const BzfWalk &walk, std::vector<typename M::Hit> &out, uint64_t *hits, uint64_t *delims)
{
    const uint32_t delim = m.delim();
    const uint64_t tiles = (w.n + BZF_TILE - 1) / BZF_TILE;
    std::vector<uint32_t> thits(tiles), tdel(tiles);
    std::vector<uint64_t> hbase(tiles), dbase(tiles);
    Group<M> g;
    *hits = *delims = 0;
    out.clear();
    if (!(tiles && (w.s_hi > w.s_lo || records))) return;
    for (uint64_t t = 0; t < tiles; t++) {
        search_front(d, w, m, records, t, g);
        uint64_t sum = 0;
        EVERY sum += g.nh[tid], tdel[t] += (uint32_t)__builtin_popcount(g.dm[tid]);
        CHECK(sum <= 4096ull * 256, "a tile's hits fit 32 bits");
        thits[t] = (uint32_t)sum;
    }
    uint64_t rh = 0, rd = 0;
    for (uint64_t t = 0; t < tiles; t++) hbase[t] = rh, dbase[t] = rd, rh += thits[t], rd += tdel[t];
    *hits = rh, *delims = rd;
    w.emit = walk.emit(rh);
    typename M::Hit unwritten;
    memset(&unwritten, 0xFF, sizeof unwritten);
    out.assign((size_t)w.emit, unwritten);
    out.shrink_to_fit();
    for (uint64_t t = 0; t < tiles && w.emit; t++) {
        if (thits[t] == 0 || hbase[t] >= w.emit) continue;
        search_front(d, w, m, records, t, g);
        uint64_t h0 = 0, dsum = 0;
        EVERY {
            const uint64_t p0 = t * BZF_TILE + tid * BZF_ITEMS;
            uint64_t rank = hbase[t] + h0;
            for (uint32_t hm = g.hm[tid]; hm; hm &= hm - 1u) {
                const uint32_t k = (uint32_t)__builtin_ctz(hm);
                if (rank >= w.emit) break;
                const uint64_t pos = p0 + k;
                uint64_t rec = 0;
                if (records) {
                    if (pos >= w.d_lo) {
                        rec = w.rec_base + dbase[t] + dsum + bzf_delims_before(g.dm[tid], k);
                    } else { // a start in the carry
                        const uint32_t gap = (uint32_t)std::min<uint64_t>(w.d_lo - pos, BZF_MAX_PATTERN);
                        uint32_t c = 0;
                        for (uint32_t j = 0; j < gap; j++) c += g.tile[tid * BZF_ITEMS + k + j] == delim;
                        rec = w.rec_base - c;
                    }
                }
                const uint64_t next = m.emit1(*g.msh, g.tile + tid * BZF_ITEMS + k, pos, w.off_base + pos, rec, out.data(), rank, w.emit);
                CHECK(next > rank && (!ONE_PER_START<M> || next == rank + 1), "a live start yields a hit, exactly one where the matcher says so");
                rank = next;
            }
            h0 += g.nh[tid], dsum += (uint32_t)__builtin_popcount(g.dm[tid]);
        }
    }
}

static inline bool same_hit(const BzfHit &a, const BzfHit &b) { return a.off == b.off && a.record == b.record; }
static inline bool same_hit(const BzmHit &a, const BzmHit &b) { return a.off == b.off && a.record == b.record && a.pattern == b.pattern && a.len == b.len; }
static inline bool ascends(const BzfHit &a, const BzfHit &b) { return a.off < b.off; }
static inline bool ascends(const BzmHit &a, const BzmHit &b) { return a.off < b.off || (a.off == b.off && a.len < b.len); }
// the hits of a call against the truth: the count whatever the room, the first `max` of them one by one, in order and none twice
template <class H>
static void same_hits(const std::vector<H> &got, const std::vector<H> &want, uint64_t nhits, uint64_t max, const char *what, uint64_t a)
{
    CHECK(nhits == want.size(), "%s (%llu): %llu hits, the truth has %zu", what, (ull)a, (ull)nhits, want.size());
    const size_t m = (size_t)std::min<uint64_t>(max, want.size());
    CHECK(got.size() >= m, "%s: %zu hits stored of %zu", what, got.size(), m);
    for (size_t i = 0; i < m; i++) {
        CHECK(same_hit(got[i], want[i]), "%s (%llu): hit %zu is (%llu, %llu), the truth (%llu, %llu), or its pattern and length differ", what, (ull)a, i, (ull)got[i].off,
              (ull)got[i].record, (ull)want[i].off, (ull)want[i].record);
        if (i) CHECK(ascends(got[i - 1], got[i]), "%s: hit %zu is out of order or a duplicate", what, i);
    }
}

// "No assertion is the zero case" (search_plan.h): beside a BzmSetWalk that never heard of assertions, a second one with
// begin_look(0, 0) said explicitly takes the same calls, and every window and lim agree field by field.
struct ZeroLookTwin {
    BzmSetWalk z;
    void begin(uint32_t plen, uint64_t front, uint64_t max, uint64_t lo, uint64_t hi, uint64_t out_start, uint64_t rec_start)
    {
        z.begin(plen, front, max, lo, hi, out_start, rec_start);
        z.begin_look(0, 0);
    }
    void window(const BzmSetWalk &walk, uint64_t bytes, bool last, const BzfWindow &w, uint64_t lim)
    {
        z.front = walk.front;
        uint64_t zl = 0;
        const BzfWindow x = z.window_set(bytes, last, &zl);
        CHECK(x.n == w.n && x.s_lo == w.s_lo && x.s_hi == w.s_hi && x.d_lo == w.d_lo && x.off_base == w.off_base && x.rank_base == w.rank_base && x.rec_base == w.rec_base &&
                  x.emit == w.emit && zl == lim,
              "begin_look(0, 0) gives another window");
        CHECK(last || z.carry_after_set(bytes) == walk.carry_after_set(bytes), "begin_look(0, 0) carries other bytes");
    }
    void advance(const BzmSetWalk &walk, uint64_t bytes, uint64_t hits, uint64_t delims, bool last)
    {
        z.advance_set(bytes, hits, delims, last);
        CHECK(z.carry == walk.carry && z.ctxb == 0 && walk.ctxb == 0 && z.out_pos == walk.out_pos && z.rank == walk.rank && z.recs == walk.recs, "begin_look(0, 0) walks on differently");
    }
};

// ---- grep_tiles and grep_scan -------------------------------------------------------------------------------------------------------
// the front of grep_tiles: the tile, the masks, the forward scan
template <class M>
static void grep_front(const uint8_t *d, const BzgWindow &w, const M &m, uint64_t t, Group<M> &g)
{
    g.stage(m, d, w.n, t);
    EVERY {
        const uint64_t p0 = t * BZF_TILE + tid * BZF_ITEMS;
        const uint32_t starts = M::BY_LIM ? bzf_range_mask16(p0, w.p_lo, w.p_hi) : bzg_starts(w, p0);
        bzg_masks(g.th[tid], w, p0, g.own[tid], m.delim(), m.match16(g.own[tid], tid, p0, g.tile, *g.msh, starts));
        bzg_local(g.th[tid], w.invert);
    }
    EVERY bzg_count_p0(*g.sh, tid, g.th[tid]);
    for (uint32_t k = 0; k < 8; k++) EVERY bzg_step_f(*g.sh, tid, k);
}
struct GrepCall { // GrepSink
    BzgWalk walk;
    uint8_t *out;  // exactly walk.cap bytes (null: not asked for)
    BzgEntry *ent; // exactly walk.max entries (null: not asked for)
    uint64_t windows;
};
// grep_window_run: d is a Text of w.n bytes, mk(w) the matcher for the window.  Returns where the tail starts
template <class MK>
static uint64_t grep_run(GrepCall &s, const uint8_t *d, const BzgWindow &w, uint64_t bytes, const MK &mk)
{
    const auto m = mk(w);
    typedef typename std::remove_const<decltype(m)>::type M;
    const uint64_t tiles = (w.n + BZF_TILE - 1) / BZF_TILE;
    uint64_t totals[BZG_TOTALS] = {0, 0, 0, w.t_lo, w.open_hit};
    s.windows++;
    if (tiles && w.p_hi > w.p_lo) {
        std::vector<BzgTile> tile(tiles);
        std::vector<BzgBase> base(tiles);
        Group<M> g;
        for (uint64_t t = 0; t < tiles; t++) {
            grep_front(d, w, m, t, g);
            EVERY bzg_count_p1(*g.sh, tid, g.th[tid], w.invert);
            for (uint32_t k = 0; k < 8; k++) EVERY bzg_step_s(*g.sh, tid, k);
            bzg_count_p2(*g.sh, tile[t]);
        }
        {
            BzgScanShared *sh = new BzgScanShared;
            memset((void *)sh, 0xAA, sizeof *sh);
            const uint32_t nt = (uint32_t)tiles;
            EVERY bzg_scan_a(*sh, tid, tile.data(), nt);
            bzg_scan_b(*sh, w, totals);
            EVERY bzg_scan_c(*sh, tid, tile.data(), nt, w);
            bzg_scan_d(*sh);
            EVERY bzg_scan_e(*sh, tid, tile.data(), nt, w);
            bzg_scan_f(*sh, totals);
            EVERY bzg_scan_g(*sh, tid, tile.data(), nt, base.data());
            delete sh;
        }
        if (s.walk.gather(totals)) {
            std::vector<BzgEntry> ent((size_t)(s.walk.want_ent ? totals[BZG_T_SEL] : 0), BzgEntry{~0ull, ~0ull, ~0ull, ~0ull});
            ent.shrink_to_fit();
            uint8_t *out = s.walk.want_out ? s.out : nullptr;
            for (uint64_t t = 0; t < tiles; t++) {
                const BzgTile &x = tile[t];
                if (x.bytes == 0) continue;
                grep_front(d, w, m, t, g);
                bool sel_first[BZF_THREADS];
                uint32_t sm[BZF_THREADS], sdm[BZF_THREADS];
                EVERY bzg_gather_p1(*g.sh, tid, g.th[tid], x, w.invert, &sel_first[tid]);
                for (uint32_t k = 0; k < 8; k++) EVERY bzg_step_b(*g.sh, tid, k);
                EVERY bzg_gather_p2(*g.sh, tid, g.th[tid], x, sel_first[tid], &sm[tid], &sdm[tid]);
                for (uint32_t k = 0; k < 8; k++) EVERY bzg_step_s(*g.sh, tid, k);
                CHECK(bzg_bytes(g.sh->s[0][BZF_THREADS - 1]) == x.bytes, "tile %llu: the gather selects %u bytes, the scan said %u", (ull)t, bzg_bytes(g.sh->s[0][BZF_THREADS - 1]),
                      x.bytes);
                uint8_t *dst = out ? out + w.out_base + base[t].out : nullptr;
                const uint32_t shift = (uint32_t)((uintptr_t)dst & 3u);
                EVERY bzg_gather_p3(*g.sh, tid, (uint32_t)t, g.th[tid], x, base[t], w, g.tile + tid * BZF_ITEMS, sm[tid], sdm[tid], shift, dst != nullptr,
                                    s.walk.want_ent ? ent.data() : nullptr);
                if (dst) EVERY bzg_gather_p4(*g.sh, tid, dst, shift, x.bytes);
            }
            for (size_t k = 0; k < ent.size(); k++) s.ent[w.sel_base + k] = ent[k];
        }
    }
    s.walk.advance(w, bytes, totals);
    return totals[BZG_T_TAIL_START];
}

struct GrepTruth { // what a program's naive split-and-find says
    Bytes out;
    std::vector<BzgEntry> ent;
    uint64_t nrecords;
};
// rooms: 0 = not asked for, 1 = above the need, 2 = the need, 3 = one below it, 4 = asked for with no room
static inline uint64_t room_of(int kind, uint64_t need) { return kind == 1 ? need + 5 : kind == 2 ? need : kind == 3 ? (need ? need - 1 : 0) : 0; }

// One grep call over the whole of `text` against the truth tr.  hold: what GrepSink gives the walk as plen; slack: the bytes behind
// a text's end; blocks: the windows' new bytes (empty: the raw call, one window over the text itself); the two rooms by kind
template <class MK>
static void grep_call(const Bytes &text, const GrepTruth &tr, const MK &mk, uint32_t hold, uint32_t invert, uint8_t slack, const std::vector<uint64_t> &blocks, int out_kind,
                      int ent_kind, uint64_t *carry_peak = nullptr, uint64_t *windows = nullptr)
{
    const uint64_t cap = room_of(out_kind, tr.out.size()), max = room_of(ent_kind, tr.ent.size());
    uint8_t *out = out_kind ? (uint8_t *)malloc(cap ? cap : 1) : nullptr; // (4-byte aligned, exactly cap bytes: cap 0 has one nobody may touch)
    std::vector<BzgEntry> ent((size_t)max);
    ent.shrink_to_fit();
    GrepCall s{BzgWalk{}, out, ent_kind ? ent.data() : nullptr, 0};
    if (ent_kind && !max) s.ent = reinterpret_cast<BzgEntry *>(sizeof(BzgEntry)); // (asked for: non-null, never dereferenced)
    s.walk.begin(hold, invert != 0, out_kind != 0, cap, ent_kind != 0, max);
    Bytes carry;
    if (blocks.empty()) {
        const Text d(text.data(), text.size(), slack);
        const uint64_t ts = grep_run(s, d.p, s.walk.window(0, text.size(), true), text.size(), mk);
        carry.assign(d.p + ts, d.p + text.size());
    } else {
        uint64_t at = 0;
        for (uint64_t bytes : blocks) {
            // GrepSink::room: a staging buffer of its own for every window, the carry in front of the new bytes
            const uint64_t extra = bzg_front_extra(s.walk.carry, BZF_FRONT), front = extra + BZF_FRONT;
            const Text stage(front + bytes, slack);
            memset(stage.p, poison_front, front);
            CHECK(carry.size() == s.walk.carry && front >= carry.size(), "the carry fits in front");
            if (!carry.empty()) memcpy(stage.p + front - carry.size(), carry.data(), carry.size());
            if (bytes) memcpy(stage.p + front, &text[at], bytes);
            at += bytes;
            const uint64_t ts = grep_run(s, stage.p, s.walk.window(front, bytes, false), bytes, mk);
            carry.assign(stage.p + ts, stage.p + front + bytes);
        }
        CHECK(at == text.size(), "the blocks are the text");
    }
    if (s.walk.held) { // GrepSink::finish: the bytes held back, where they lie
        CHECK(carry.size() == s.walk.carry, "the carry");
        const Text held(carry.data(), carry.size(), slack);
        const uint64_t ts = grep_run(s, held.p, s.walk.window(s.walk.carry, 0, true), 0, mk);
        carry.erase(carry.begin(), carry.begin() + ts);
    }
    CHECK(carry.size() == s.walk.carry && s.walk.held == 0, "the tail");
    bool copy, entry;
    s.walk.tail_rooms(&copy, &entry);
    const BzgEntry te = s.walk.tail_entry();
    if (copy && !carry.empty()) memcpy(s.out + s.walk.out_bytes, carry.data(), carry.size());
    s.walk.tail_done();
    if (entry) s.ent[s.walk.sel - 1] = te;
    CHECK(s.walk.sel == tr.ent.size() && s.walk.out_bytes == tr.out.size() && s.walk.nrecords() == tr.nrecords,
          "grep counts: %llu selected of %llu bytes, %llu records; the truth %zu, %zu, %llu", (ull)s.walk.sel, (ull)s.walk.out_bytes, (ull)s.walk.nrecords(), tr.ent.size(),
          tr.out.size(), (ull)tr.nrecords);
    const bool over = (out_kind && tr.out.size() > cap) || (ent_kind && tr.ent.size() > max);
    CHECK(s.walk.overflow() == over, "BZH_E_CAP exactly when a room that is asked for is too small");
    if (!over) {
        if (out_kind && !tr.out.empty()) CHECK(memcmp(out, tr.out.data(), tr.out.size()) == 0, "the selected bytes");
        for (size_t k = 0; ent_kind && k < tr.ent.size(); k++)
            CHECK(ent[k].record == tr.ent[k].record && ent[k].off == tr.ent[k].off && ent[k].len == tr.ent[k].len && ent[k].out_off == tr.ent[k].out_off,
                  "grep entry %zu: record %llu off %llu len %llu out_off %llu, the truth %llu %llu %llu %llu", k, (ull)ent[k].record, (ull)ent[k].off, (ull)ent[k].len,
                  (ull)ent[k].out_off, (ull)tr.ent[k].record, (ull)tr.ent[k].off, (ull)tr.ent[k].len, (ull)tr.ent[k].out_off);
    }
    if (carry_peak) *carry_peak = std::max(*carry_peak, s.walk.carry_peak);
    if (windows) *windows = s.windows;
    free(out);
}

#endif // BZH_SCAN_HOST_H
