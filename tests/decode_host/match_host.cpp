// match_host.cpp -- the matched parts alone (bzh_match*) without a device, built with g++ -fsanitize=address,undefined.
// (a) The phases of banzai_amd/csrc/match_core.h -- pass one with the matcher's longest1, the scan of the maps, the counting pass,
//     the sums, the gather -- run thread by thread and tile by tile in the kernels' layout, behind the tile front the kernels
//     compile (scan_host.h's Group), against a ten-line greedy loop.  Every text is allocated as the kernels' contract states and
//     every table has its exact size, so a read or a store outside is a sanitizer report.  Three matchers: one string, a set with a
//     pattern that is a prefix of another, an automaton with spans 1 and 256.
// (b) The windows and the cursor of banzai_amd/csrc/match_plan.h with (a) as the device: blocks of seeded sizes, a staging buffer
//     allocated anew for every window, against the same truth.
//
//   match_host <seed> <cases>     exit status 0: everything held
#define HOST_NAME "match_host"
#include <functional>
#include <string>

#include "../../include/bzhip.h"
#include "../../banzai_amd/csrc/regex_core.h"
#include "../../banzai_amd/csrc/regex_plan.h"
#include "../../banzai_amd/csrc/patset_plan.h"
#include "scan_host.h"
#include "../../banzai_amd/csrc/match_core.h"

static_assert(sizeof(bzh_match_entry) == sizeof(MtEntry) && sizeof(MtEntry) == 32, "an entry is four words");

typedef std::vector<Bytes> Pats;
static Bytes B(const char *s) { return Bytes(s, s + strlen(s)); }

// ---- what is looked for: the matcher for a window, and the rule without a tile -----------------------------------------------------
struct Tables { // a compiled set or automaton as the device holds it
    uint8_t *cls = nullptr;
    uint16_t *first = nullptr, *table = nullptr;
    uint32_t *pat_no = nullptr;
    uint32_t classes = 0, nterm = 0, max_len = 0, states = 0;
    ~Tables() { free(cls), free(first), free(table), free(pat_no); }
    // the longest match at text[s ..) that ends at or in front of n (0: none), walked without a tile
    uint32_t longest(const Bytes &text, uint64_t s, uint32_t *pattern) const
    {
        uint32_t st = 0, best = 0;
        for (uint32_t depth = 0; s + depth < text.size() && depth < max_len; depth++) {
            const size_t at = (size_t)st * classes + cls[text[s + depth]];
            st = depth == 0 ? first[text[s]] : table[at];
            if (!st) break;
            if (st <= nterm) best = depth + 1, *pattern = pat_no[st - 1];
        }
        return best;
    }
};
struct What {
    std::string name;
    Bytes one;        // a single string, or
    Tables t;         // ... a set or an automaton
    bool is_auto = false;
    uint32_t delim = '\n';
    uint32_t plen() const { return one.empty() ? t.max_len : (uint32_t)one.size(); }
    uint32_t longest(const Bytes &text, uint64_t s, uint32_t *pattern) const
    {
        if (one.empty()) return t.longest(text, s, pattern);
        *pattern = 0;
        return s + one.size() <= text.size() && memcmp(&text[s], one.data(), one.size()) == 0 ? (uint32_t)one.size() : 0;
    }
};
static void what_set(What &q, const Pats &pats)
{
    BzmPlan plan;
    std::vector<const uint8_t *> ptr;
    std::vector<size_t> len;
    for (const Bytes &p : pats) ptr.push_back(p.data()), len.push_back(p.size());
    char err[200] = "";
    CHECK(bzm_compile(ptr.data(), len.data(), pats.size(), 0, plan, err, sizeof err), "the set compiles: %s", err);
    q.t.cls = exact(plan.cls, 256), q.t.first = exact(plan.first, 256);
    q.t.table = exact(plan.table.data(), plan.table.size()), q.t.pat_no = exact(plan.pat_no.data(), plan.pat_no.size());
    q.t.classes = plan.classes, q.t.nterm = (uint32_t)plan.distinct, q.t.max_len = plan.max_len, q.t.states = plan.states;
}
static void what_auto(What &q, const Pats &exprs, uint32_t span)
{
    BzrPlan plan;
    std::vector<const uint8_t *> ptr;
    std::vector<size_t> len;
    for (const Bytes &p : exprs) ptr.push_back(p.data()), len.push_back(p.size());
    char err[200] = "";
    CHECK(bzr_compile(ptr.data(), len.data(), exprs.size(), 0, span, plan, err, sizeof err), "the automaton compiles: %s", err);
    q.t.cls = exact(plan.cls, 256), q.t.first = exact(plan.first, 256);
    q.t.table = exact(plan.table.data(), plan.table.size()), q.t.pat_no = exact(plan.pat_no.data(), plan.pat_no.size());
    q.t.classes = plan.classes, q.t.nterm = plan.nterm, q.t.max_len = plan.max_len, q.t.states = plan.states;
    q.is_auto = true;
}

// ---- the truth: the ten-line greedy loop -------------------------------------------------------------------------------------------
struct Truth {
    Bytes out;
    std::vector<MtEntry> ent;
    uint64_t candidates = 0;
};
static Truth greedy(const Bytes &text, const What &q, bool records)
{
    Truth tr;
    uint64_t cursor = 0, rec = 0;
    for (uint64_t s = 0; s < text.size(); s++) {
        uint32_t pattern = 0;
        const uint32_t l = s >= cursor ? q.longest(text, s, &pattern) : 0;
        if (l) {
            tr.ent.push_back(MtEntry{s, records ? rec : 0, pattern, l, tr.out.size()});
            tr.out.insert(tr.out.end(), text.begin() + s, text.begin() + s + l);
            cursor = s + l;
        }
        rec += text[s] == q.delim;
    }
    return tr;
}

// ---- (a) the device: match_window_run of match.hip, phase by phase -------------------------------------------------------------------
struct MatchCall { // MatchSink
    MtWalk walk;
    uint8_t *out;
    MtEntry *ent;
    bool records;
    uint64_t windows = 0;
};
static void levels(MtShared &sh, const uint32_t *hm, const BzfVec *len)
{
    EVERY mt_local(sh, tid, hm[tid], len[tid]);
    for (uint32_t r = 0; r < 4; r++) EVERY mt_group_step(sh, tid, r);
}
static void sums(MtShared &sh)
{
    for (uint32_t k = 0; k < 8; k++) EVERY mt_sum_step(sh, tid, k);
}
template <class M>
static void match_run(MatchCall &s, const uint8_t *d, const MtWindow &mw, uint64_t bytes, bool last, const M &m)
{
    const BzfWindow &w = mw.w;
    const uint64_t tiles = (w.n + BZF_TILE - 1) / BZF_TILE;
    const uint32_t nt = (uint32_t)tiles;
    uint64_t totals[MT_TOTALS] = {0, 0, 0, 0, 0, 0, 0};
    s.windows++;
    if (s.walk.runs(mw, s.records)) {
        std::vector<MtTile> tile(tiles);
        std::vector<MtCount> cnt(tiles);
        std::vector<MtBase> base(tiles);
        std::vector<uint16_t> hits(tiles * BZF_THREADS);
        std::vector<uint8_t> map(tiles * 256, 0xAA), summ(256 * 256, 0xAA);
        uint8_t *lens;
        if (posix_memalign((void **)&lens, 16, tiles * BZF_TILE)) abort();
        memset(lens, 0xFF, tiles * BZF_TILE); // (what no thread stores is the longest length: a read of it shows)
        Group<M> g;
        MtShared *sh = new MtShared;
        uint32_t hm[BZF_THREADS];
        BzfVec len[BZF_THREADS];
        for (uint64_t t = 0; t < tiles; t++) { // match_tiles
            g.stage(m, d, w.n, t);
            memset((void *)sh, 0xAA, sizeof *sh);
            EVERY mt_init(*sh, tid);
            EVERY {
                const uint64_t p0 = t * BZF_TILE + tid * BZF_ITEMS;
                hm[tid] = m.match16(g.own[tid], tid, p0, g.tile, *g.msh, bzf_range_mask16(p0, w.s_lo, w.s_hi));
                uint8_t l[16] = {0};
                for (uint32_t v = hm[tid]; v; v &= v - 1u) {
                    const uint32_t k = (uint32_t)__builtin_ctz(v);
                    uint32_t pattern;
                    const uint32_t got = m.longest1(*g.msh, g.tile + tid * BZF_ITEMS + k, p0 + k, &pattern);
                    CHECK(got >= 1 && got <= 256, "a start that match16 names has a longest match");
                    l[k] = (uint8_t)(got - 1);
                }
                memcpy(&len[tid], l, 16);
                hits[t * BZF_THREADS + tid] = (uint16_t)hm[tid];
                if (hm[tid]) memcpy(lens + p0, l, 16), sh->any = 1;
                const BzfVec &v = g.own[tid];
                const uint32_t dm = s.records ? bzf_eq_mask16(v.x, v.y, v.z, v.w, m.delim()) & bzf_range_mask16(p0, w.d_lo, w.n) : 0u;
                mt_sum_put(*sh, tid, (uint32_t)__builtin_popcount(hm[tid]), 0, (uint32_t)__builtin_popcount(dm));
            }
            sums(*sh);
            MtTile o{mt_s_cnt(mt_sum_all(*sh)), mt_s_del(mt_sum_all(*sh)), MT_CONST, 0};
            if (sh->any) {
                levels(*sh, hm, len);
                EVERY mt_map(*sh, tid);
                EVERY mt_map_open(*sh, tid);
                if (sh->open) {
                    EVERY map[t * 256 + tid] = sh->map[tid];
                    o.konst = 0;
                } else {
                    o.konst = MT_CONST | sh->map[0];
                }
            }
            tile[t] = o;
        }
        { // match_scan
            MtScanShared *ss = new MtScanShared;
            memset((void *)ss, 0xAA, sizeof *ss);
            EVERY mt_scan_a(*ss, tid, tile.data(), map.data(), nt, summ.data());
            mt_scan_b(*ss, summ.data(), totals);
            EVERY mt_scan_c(*ss, tid, tile.data(), map.data(), nt, base.data());
            mt_scan_d(*ss, totals);
            delete ss;
        }
        auto select_front = [&](uint64_t t, uint32_t *sm, uint32_t *nb, uint32_t *le) { // match_select up to the marks
            memset((void *)sh, 0xAA, sizeof *sh);
            EVERY mt_init(*sh, tid);
            EVERY {
                hm[tid] = hits[t * BZF_THREADS + tid];
                memset(&len[tid], 0, 16);
                if (hm[tid]) memcpy(&len[tid], lens + t * BZF_TILE + tid * BZF_ITEMS, 16);
            }
            levels(*sh, hm, len);
            mt_group_entries(*sh, tile[t].entry);
            for (uint32_t gq = 0; gq < BZF_TILE / MT_GROUP; gq++) mt_seg_entries(*sh, gq);
            EVERY sm[tid] = mt_marks(*sh, tid, hm[tid], len[tid], &nb[tid], &le[tid]);
        };
        uint32_t sm[BZF_THREADS], nb[BZF_THREADS], le[BZF_THREADS];
        for (uint64_t t = 0; t < tiles; t++) { // match_select<false>
            if (tile[t].cand == 0) {
                cnt[t] = MtCount{0, 0, 0, 0};
                continue;
            }
            select_front(t, sm, nb, le);
            EVERY mt_sum_put(*sh, tid, (uint32_t)__builtin_popcount(sm[tid]), nb[tid], 0);
            sums(*sh);
            EVERY mt_last_end(*sh, tid, sm[tid], le[tid]);
            cnt[t] = MtCount{mt_s_cnt(mt_sum_all(*sh)), mt_s_bytes(mt_sum_all(*sh)), sh->last_end, 0};
        }
        { // match_sum
            MtSumShared *ss = new MtSumShared;
            memset((void *)ss, 0xAA, sizeof *ss);
            EVERY mt_sum_a(*ss, tid, cnt.data(), nt);
            mt_sum_b(*ss, totals);
            EVERY mt_sum_c(*ss, tid, cnt.data(), nt, base.data());
            delete ss;
        }
        if (s.walk.gather(totals)) { // match_select<true>
            std::vector<MtEntry> ent((size_t)(s.walk.want_ent ? totals[MT_T_SEL] : 0), MtEntry{~0ull, ~0ull, ~0u, ~0u, ~0ull});
            ent.shrink_to_fit();
            uint8_t *out = s.walk.want_out ? s.out : nullptr;
            for (uint64_t t = 0; t < tiles; t++) {
                if (cnt[t].bytes == 0) continue;
                g.stage(m, d, w.n, t);
                select_front(t, sm, nb, le);
                uint32_t dm[BZF_THREADS];
                EVERY {
                    const uint64_t p0 = t * BZF_TILE + tid * BZF_ITEMS;
                    const BzfVec &v = g.own[tid];
                    dm[tid] = s.records ? bzf_eq_mask16(v.x, v.y, v.z, v.w, m.delim()) & bzf_range_mask16(p0, w.d_lo, w.n) : 0u;
                    mt_sum_put(*sh, tid, (uint32_t)__builtin_popcount(sm[tid]), nb[tid], (uint32_t)__builtin_popcount(dm[tid]));
                }
                sums(*sh);
                CHECK(mt_s_bytes(mt_sum_all(*sh)) == cnt[t].bytes && mt_s_cnt(mt_sum_all(*sh)) == cnt[t].cnt, "tile %llu: the gather selects what the count said", (ull)t);
                uint8_t *comp = reinterpret_cast<uint8_t *>(sh->y);
                uint64_t s0[BZF_THREADS];
                EVERY s0[tid] = mt_sum_excl(*sh, tid); // (read before the compaction overwrites nothing of s: it lies beside y)
                EVERY mt_gather(m, *g.msh, comp, sm[tid], len[tid], dm[tid], s0[tid], g.tile + tid * BZF_ITEMS, t * BZF_TILE + tid * BZF_ITEMS, w, s.records ? 1u : 0u,
                                base[t], mw.out_base, out != nullptr, s.walk.want_ent ? ent.data() : nullptr);
                if (out) EVERY mt_store(comp, tid, out + mw.out_base + base[t].bytes, cnt[t].bytes);
            }
            for (size_t k = 0; k < ent.size(); k++) s.ent[w.rank_base + k] = ent[k];
        }
        delete sh;
        free(lens);
    }
    s.walk.advance(mw, bytes, totals, last);
}

// the matcher of a window, as pick_matcher makes it
template <class F>
static void with_matcher(const What &q, const MtWindow &mw, F &&f)
{
    if (!q.one.empty()) return f(BzfOne{{}, bzf_pattern(q.one.data(), (uint32_t)q.one.size(), q.delim)});
    const BzmSet set{q.t.cls, q.t.first, q.t.table, q.t.pat_no, q.t.classes, q.t.nterm, q.t.max_len, q.delim, mw.lim};
    if (!q.is_auto) return f(BzmMatcher{set});
    const BzrAuto a{set, q.t.states * q.t.classes};
    if (a.entries <= BZR_LDS_ROWS) f(BzrMatcher<true, false>{{a}, {}});
    else f(BzrMatcher<false, false>{{a}, {}});
}

struct Stats {
    uint64_t entered, open, windows;
};
// One call over the whole of `text` against the greedy loop.  blocks: the windows' new bytes (empty: the raw call, one window over
// the text itself); the two rooms by kind (scan_host.h: room_of)
static Stats match_call(const Bytes &text, const What &q, bool records, const std::vector<uint64_t> &blocks, int out_kind, int ent_kind, const char *what)
{
    const Truth tr = greedy(text, q, records);
    const uint64_t cap = room_of(out_kind, tr.out.size()), max = room_of(ent_kind, tr.ent.size());
    uint8_t *out = out_kind ? (uint8_t *)malloc(cap ? cap : 1) : nullptr;
    std::vector<MtEntry> ent((size_t)max);
    ent.shrink_to_fit();
    MatchCall s{MtWalk{}, out, ent_kind ? ent.data() : nullptr, records};
    if (ent_kind && !max) s.ent = reinterpret_cast<MtEntry *>(sizeof(MtEntry)); // (asked for: non-null, never dereferenced)
    s.walk.begin(q.plen(), 0, 0, q.one.empty(), out_kind != 0, cap, ent_kind != 0, max);
    const uint8_t slack = 0xEE;
    if (blocks.empty()) {
        const Text d(text.data(), text.size(), slack);
        const MtWindow mw = s.walk.window(0, text.size(), true);
        with_matcher(q, mw, [&](const auto &m) { match_run(s, d.p, mw, text.size(), true, m); });
    } else {
        Bytes carry;
        uint64_t at = 0;
        for (uint64_t bytes : blocks) { // MatchSink::room and window: a staging buffer of its own for every window
            const uint64_t front = BZF_FRONT;
            CHECK(carry.size() == s.walk.walk.carry && carry.size() <= front, "the carry fits in front");
            const Text stage(front + bytes, slack);
            memset(stage.p, poison_front, front);
            if (!carry.empty()) memcpy(stage.p + front - carry.size(), carry.data(), carry.size());
            if (bytes) memcpy(stage.p + front, &text[at], bytes);
            at += bytes;
            const MtWindow mw = s.walk.window(front, bytes, false);
            const uint64_t keep = s.walk.carry_after(bytes);
            carry.assign(stage.p + mw.w.n - keep, stage.p + mw.w.n);
            with_matcher(q, mw, [&](const auto &m) { match_run(s, stage.p, mw, bytes, false, m); });
        }
        CHECK(at == text.size(), "the blocks are the text");
        if (s.walk.walk.carry) { // MatchSink::finish
            CHECK(carry.size() == s.walk.walk.carry, "the carry");
            const Text held(carry.data(), carry.size(), slack);
            const MtWindow mw = s.walk.window(carry.size(), 0, true);
            with_matcher(q, mw, [&](const auto &m) { match_run(s, held.p, mw, 0, true, m); });
        }
    }
    CHECK(s.walk.sel == tr.ent.size() && s.walk.out_bytes == tr.out.size(), "%s (%s, n %zu): %llu matches of %llu bytes, the truth %zu of %zu", what, q.name.c_str(), text.size(),
          (ull)s.walk.sel, (ull)s.walk.out_bytes, tr.ent.size(), tr.out.size());
    const bool over = (out_kind && tr.out.size() > cap) || (ent_kind && tr.ent.size() > max);
    CHECK(s.walk.overflow() == over, "%s: BZH_E_CAP exactly when a room that is asked for is too small", what);
    if (!over) {
        if (out_kind && !tr.out.empty()) CHECK(memcmp(out, tr.out.data(), tr.out.size()) == 0, "%s (%s, n %zu): the matched bytes", what, q.name.c_str(), text.size());
        for (size_t k = 0; ent_kind && k < tr.ent.size(); k++) {
            const MtEntry &a = ent[k], &b = tr.ent[k];
            CHECK(a.off == b.off && a.record == b.record && a.pattern == b.pattern && a.len == b.len && a.out_off == b.out_off,
                  "%s (%s, n %zu): entry %zu is off %llu record %llu pattern %u len %u out_off %llu, the truth %llu %llu %u %u %llu", what, q.name.c_str(), text.size(), k,
                  (ull)a.off, (ull)a.record, a.pattern, a.len, (ull)a.out_off, (ull)b.off, (ull)b.record, b.pattern, b.len, (ull)b.out_off);
        }
    }
    free(out);
    return Stats{s.walk.entered, s.walk.open, s.windows};
}

static Bytes random_text(uint64_t n, const char *alphabet)
{
    Bytes t(n);
    const size_t k = strlen(alphabet);
    for (auto &b : t) b = (uint8_t)alphabet[below(k)];
    return t;
}

int main(int argc, char **argv)
{
    rng_state = argc > 1 ? strtoull(argv[1], nullptr, 10) * 0x9E3779B97F4A7C15ull + 1 : 1;
    const uint64_t cases = argc > 2 ? strtoull(argv[2], nullptr, 10) : 600;

    What one, one256, set, auto256, auto1;
    one.name = "aa", one.one = B("aa");
    one256.name = "a x 256", one256.one = Bytes(256, 'a');
    set.name = "{a, ab, abb, b1}";
    what_set(set, {B("a"), B("ab"), B("abb"), B("b1")});
    auto256.name = "a+b?|[0-9]+ span 256";
    what_auto(auto256, {B("a+b?"), B("[0-9]+")}, 256);
    auto1.name = "a+|b span 1";
    what_auto(auto1, {B("a+"), B("b")}, 1);
    const What *all[] = {&one, &set, &auto256, &auto1};

    // ---- (a) raw: one window over the text
    uint64_t raw = 0;
    const uint64_t sizes[] = {0, 1, 15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 8192, 12289};
    for (uint64_t n : sizes)
        for (const What *q : all)
            for (int dense = 0; dense < 3; dense++) {
                const Bytes text = random_text(n, dense == 0 ? "aab b1\n" : dense == 1 ? "aaaaaab1\n" : "xyz  a\n\n");
                match_call(text, *q, (raw & 1) != 0, {}, 1, 1, "raw");
                raw++;
            }
    { // sparse: no tile is entered beyond its first byte, none is open
        Bytes text = random_text(12289, "xyz \n");
        text[5000] = 'a', text[5001] = 'a';
        const Stats st = match_call(text, one, true, {}, 1, 1, "sparse");
        CHECK(st.entered == 0 && st.open == 0, "a sparse text enters %llu tiles and opens %llu", (ull)st.entered, (ull)st.open);
        raw++;
    }
    for (uint64_t begin : {4u, 7u}) { // a run of one byte over three tiles searched for two of it: every tile of the run is open, both parities cross both edges
        Bytes text(begin, 'x');
        text.resize(begin + 3 * BZF_TILE, 'a');
        text.resize(text.size() + 100, 'y');
        const Stats st = match_call(text, one, false, {}, 1, 1, "a run searched for two");
        CHECK(st.open >= 3, "every tile of a run is open: %llu", (ull)st.open);
        CHECK((begin & 1) == 0 || st.entered >= 1, "an odd run enters a tile beyond its first byte");
        raw++;
    }
    for (uint64_t begin : {0u, 1u, 255u}) { // the same for a 256-byte pattern: entries up to 255
        Bytes text(begin, 'x');
        text.resize(begin + 3 * BZF_TILE + 77, 'a');
        const Stats st = match_call(text, one256, false, {}, 1, 1, "a run searched for 256");
        CHECK(st.open >= 2 && (begin == 0 || st.entered >= 2), "a run of 256s: %llu open, %llu entered", (ull)st.open, (ull)st.entered);
        raw++;
    }
    { // a tile entered at 255: 256 a's from the last byte of tile 0
        Bytes text(3 * BZF_TILE, 'x');
        for (uint32_t k = 0; k < 256; k++) text[BZF_TILE - 1 + k] = 'a';
        const Stats st = match_call(text, one256, false, {}, 1, 1, "entered at 255");
        CHECK(st.entered == 1, "one tile is entered: %llu", (ull)st.entered);
        raw++;
    }
    { // a match that spans a tile edge and is selected; one that spans it and is dropped because the cursor lies inside it
        Bytes text(2 * BZF_TILE + 10, 'x');
        text[BZF_TILE - 1] = 'a', text[BZF_TILE] = 'a';                                   // selected across the edge
        text[2 * BZF_TILE - 2] = 'a', text[2 * BZF_TILE - 1] = 'a', text[2 * BZF_TILE] = 'a'; // aa at -2 selected, aa at -1 dropped
        const Stats st = match_call(text, one, true, {}, 1, 1, "across an edge");
        CHECK(st.entered == 1, "the selected match enters the next tile: %llu", (ull)st.entered);
        raw++;
    }
    for (uint64_t tiles : {300u, 700u}) { // a scan thread owns several tiles: a dense stretch across chunk edges, a chunk with no constant tile
        Bytes text = random_text(tiles * BZF_TILE - 333, "xyz ab1\n");
        for (uint64_t p = 3 * BZF_TILE + 5; p < 13 * BZF_TILE + 6; p++) text[p] = 'a';
        for (uint64_t p = (tiles - 20) * BZF_TILE - 9; p < (tiles - 11) * BZF_TILE + 1; p++) text[p] = 'a';
        for (const What *q : {(const What *)&one, (const What *)&one256, (const What *)&set}) {
            const Stats st = match_call(text, *q, true, {}, 1, 1, "many tiles");
            CHECK(q == &set || (st.open >= 16 && st.entered >= 1), "many tiles: %llu open, %llu entered", (ull)st.open, (ull)st.entered);
            raw++;
        }
    }
    printf("raw: %llu cases held\n", (ull)raw);

    // ---- (b) the windows
    uint64_t beyond = 0, multi = 0;
    for (uint64_t c = 0; c < cases; c++) {
        const What *q = c % 7 == 6 ? &one256 : all[c % 4];
        const uint64_t nblocks = 1 + below(7);
        std::vector<uint64_t> sizes_b;
        uint64_t n = 0;
        for (uint64_t k = 0; k < nblocks; k++) {
            const uint64_t kind = below(6);
            const uint64_t b = kind == 0 ? below(4) : kind == 1 ? 1 + below(300) : kind == 2 ? BZF_TILE - 2 + below(5) : 1 + below(3 * BZF_TILE);
            sizes_b.push_back(b), n += b;
        }
        Bytes text = random_text(n, c % 3 == 0 ? "aab b1\n" : c % 3 == 1 ? "aaaaaaab\n" : "xyz  ab1\n");
        if (c % 5 == 0) std::fill(text.begin(), text.end(), 'a'); // a dense run across every window edge
        std::vector<uint64_t> blocks; // windows of 1 to 4 blocks
        for (size_t k = 0; k < sizes_b.size();) {
            uint64_t take = 1 + below(4), sum = 0;
            for (; take && k < sizes_b.size(); take--, k++) sum += sizes_b[k];
            blocks.push_back(sum);
        }
        static const int kinds[][2] = {{1, 1}, {2, 2}, {3, 1}, {1, 3}, {4, 4}, {0, 0}, {0, 1}, {1, 0}, {2, 1}};
        const int *rk = kinds[c % 9];
        const Stats st = match_call(text, *q, (c & 1) != 0, blocks, rk[0], rk[1], "windows");
        multi += st.windows > 1;
        beyond += c % 5 == 0 && blocks.size() > 1;
        if (c % 11 == 0) match_call(text, *q, (c & 1) != 0, {}, 1, 1, "the same text raw");
    }
    CHECK(cases < 50 || (multi > cases / 4 && beyond > 0), "the seeded cases cross window edges: %llu of %llu, %llu dense", (ull)multi, (ull)cases, (ull)beyond);
    printf("windows: %llu cases held\n", (ull)cases);
    return 0;
}
