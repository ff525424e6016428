// grep_ctx_host.cpp -- the grep with context records without a device, built with g++ -fsanitize=address,undefined.
// (a) The phases of banzai_amd/csrc/grep_ctx_core.h -- pass one, scan one, pass two, scan two, the gather -- run thread by thread
//     and tile by tile in the kernels' layout, behind the tile front the kernels compile (scan_host.h's Group over BzfOne), against a
//     naive split-find-dilate.  Every text is allocated as the kernels' contract states and every other buffer has its exact size,
//     so a read or a store outside is a sanitizer report.  With context 0, 0 the same inputs also go through grep_core.h's phases
//     (scan_host.h's grep_call) against the same truth: the two sets of phases give the same bytes and entries.
// (b) The windows, the pending records and the tail (banzai_amd/csrc/grep_ctx_plan.h), with (a) as the device: blocks of seeded
//     sizes, a staging buffer allocated anew for every window, against the same truth; pending_peak against a count of its own.
//
//   grep_ctx_host <seed> <cases>     exit status 0: everything held
#define HOST_NAME "grep_ctx_host"
#include "../../include/bzhip.h"
#include "scan_host.h"
#include "../../banzai_amd/csrc/grep_ctx_plan.h"

struct Pattern {
    uint8_t pat[BZF_MAX_PATTERN];
    uint32_t plen, delim, invert;
};
static uint8_t slack_of(const Pattern &p) { return p.delim == 0xEE ? 0xED : 0xEE; }

// ---- the truth: split, find, dilate -------------------------------------------------------------------------------------------------
struct CtxTruth {
    Bytes out;
    std::vector<BzgEntry> ent; // len with bit 63 on context records
    std::vector<uint64_t> end; // of every record
    std::vector<uint8_t> prim;
    uint64_t nrecords = 0, matched = 0, context = 0, groups = 0;
};
static CtxTruth naive(const Bytes &text, const Pattern &p, uint32_t B, uint32_t A)
{
    CtxTruth tr;
    const uint64_t n = text.size();
    uint64_t start = 0;
    auto close = [&](uint64_t end) {
        bool hit = false;
        for (uint64_t s = start; s < end && !hit; s++) hit = s + p.plen <= n && memcmp(&text[s], p.pat, p.plen) == 0;
        tr.prim.push_back(hit != (p.invert != 0));
        tr.end.push_back(end);
        start = end;
    };
    for (uint64_t i = 0; i < n; i++)
        if (text[i] == p.delim) close(i + 1);
    if (start < n) close(n);
    const uint64_t R = tr.nrecords = tr.prim.size();
    std::vector<uint8_t> sel(R, 0);
    for (uint64_t r = 0; r < R; r++)
        if (tr.prim[r]) {
            const uint64_t lo = r > B ? r - B : 0, hi = std::min<uint64_t>(R - 1, r + (uint64_t)A);
            for (uint64_t j = lo; j <= hi; j++) sel[j] = 1;
            tr.matched++;
        }
    for (uint64_t r = 0; r < R; r++) {
        if (!sel[r]) continue;
        const uint64_t s = r ? tr.end[r - 1] : 0, len = tr.end[r] - s;
        tr.ent.push_back(BzgEntry{r, s, len | (tr.prim[r] ? 0 : BZC_LEN_CONTEXT), tr.out.size()});
        tr.out.insert(tr.out.end(), text.begin() + s, text.begin() + tr.end[r]);
        tr.context += !tr.prim[r];
        tr.groups += r == 0 || !sel[r - 1];
    }
    return tr;
}
// the records a window edge leaves pending: `done` bytes of the text are processed
static uint64_t pending_truth(const CtxTruth &tr, const Bytes &text, uint32_t delim, uint64_t done, uint32_t B, uint32_t A)
{
    uint64_t closed = 0;
    while (closed < tr.end.size() && tr.end[closed] <= done && text[tr.end[closed] - 1] == delim) closed++;
    uint64_t g = 0;
    while (g < closed && !tr.prim[closed - 1 - g]) g++;
    if (g == closed) return std::min<uint64_t>(B, closed); // no primary so far
    return g > A ? std::min<uint64_t>(B, g - A) : 0;
}

// ---- (a) the device: grep_ctx_window_run of grep.hip, phase by phase ------------------------------------------------------------------
struct CtxCall { // GrepSink
    BzcWalk walk;
    uint8_t *out;
    BzgEntry *ent;
    uint64_t windows;
};
static void ctx_front(const uint8_t *d, const BzcWindow &w, uint32_t delim, uint64_t t, Group<BzfOne> &g, BzcShared &sh, const uint16_t *hits)
{
    EVERY {
        const uint64_t p0 = t * BZF_TILE + tid * BZF_ITEMS;
        g.own[tid] = bzf_load16(d, w.w.n, p0);
        *reinterpret_cast<BzfVec *>(g.tile + tid * BZF_ITEMS) = g.own[tid];
        bzc_masks(g.th[tid], w, p0, g.own[tid], delim, hits[t * BZF_THREADS + tid]);
    }
    EVERY bzg_count_p0(sh.g, tid, g.th[tid]);
    for (uint32_t k = 0; k < 8; k++) EVERY bzg_step_f(sh.g, tid, k);
}
static uint64_t ctx_run(CtxCall &s, const uint8_t *d, const BzcWindow &w, uint64_t bytes, const BzfOne &m)
{
    const uint64_t tiles = (w.w.n + BZF_TILE - 1) / BZF_TILE;
    uint64_t totals[BZC_TOTALS];
    s.walk.totals_idle(w, totals);
    s.windows++;
    if (s.walk.runs(w)) {
        std::vector<BzcTile> tile(tiles);
        std::vector<BzcCount> cnt(tiles);
        std::vector<BzgBase> base(tiles);
        std::vector<uint16_t> table(tiles * BZF_THREADS);
        uint16_t *hits = table.data();
        Group<BzfOne> g;
        BzcShared *sh = new BzcShared;
        const uint32_t nt = (uint32_t)tiles;
        for (uint64_t t = 0; t < tiles; t++) { // pass one
            g.stage(m, d, w.w.n, t);
            memset((void *)sh, 0xAA, sizeof *sh);
            EVERY {
                const uint64_t p0 = t * BZF_TILE + tid * BZF_ITEMS;
                const uint32_t hm = m.match16(g.own[tid], tid, p0, g.tile, *g.msh, bzg_starts(w.w, p0));
                hits[t * BZF_THREADS + tid] = (uint16_t)hm;
                bzc_masks(g.th[tid], w, p0, g.own[tid], m.delim(), hm);
            }
            EVERY bzg_count_p0(sh->g, tid, g.th[tid]);
            for (uint32_t k = 0; k < 8; k++) EVERY bzg_step_f(sh->g, tid, k);
            EVERY bzc_count_p1(*sh, tid, g.th[tid], w, t * BZF_TILE + tid * BZF_ITEMS);
            for (uint32_t k = 0; k < 8; k++) {
                EVERY bzc_step(*sh, tid, k);
                EVERY bzg_step_s(sh->g, tid, k);
            }
            bzc_count_p2(*sh, tile[t]);
        }
        { // scan one
            BzcScanShared *ss = new BzcScanShared;
            memset((void *)ss, 0xAA, sizeof *ss);
            EVERY bzc_scan_a(*ss, tid, tile.data(), nt, w);
            bzc_scan_b(*ss, w, totals);
            EVERY bzc_scan_c(*ss, tid, tile.data(), nt, w, base.data());
            bzc_scan_d(*ss, w, totals);
            EVERY bzc_scan_e(*ss, tid, tile.data(), nt, w);
            delete ss;
        }
        BzcSel sel[BZF_THREADS];
        uint32_t pm[BZF_THREADS];
        auto select = [&](uint64_t t) {
            memset((void *)sh, 0xAA, sizeof *sh);
            ctx_front(d, w, m.delim(), t, g, *sh, hits);
            EVERY pm[tid] = bzc_sel_p1(*sh, tid, g.th[tid], tile[t], w, t * BZF_TILE + tid * BZF_ITEMS);
            for (uint32_t k = 0; k < 8; k++) EVERY bzc_step(*sh, tid, k);
            const bool first_rec = w.w.rec_base == 0 && base[t].del == 0;
            EVERY sel[tid] = bzc_sel_p2(*sh, tid, g.th[tid], pm[tid], tile[t], w, first_rec, t * BZF_TILE + tid * BZF_ITEMS, totals[BZC_T_PEND_FIND],
                                        totals[BZG_T_DEL] - base[t].del - tile[t].nd, &totals[BZC_T_PEND_START]);
        };
        for (uint64_t t = 0; t < tiles; t++) { // pass two
            select(t);
            EVERY bzc_count2_p3(*sh, tid, sel[tid]);
            for (uint32_t k = 0; k < 8; k++) EVERY bzg_step_s(sh->g, tid, k);
            bzc_count2_p4(*sh, cnt[t]);
        }
        { // scan two
            BzcSumShared *ss = new BzcSumShared;
            memset((void *)ss, 0xAA, sizeof *ss);
            EVERY bzc_sum_a(*ss, tid, cnt.data(), nt);
            bzc_sum_b(*ss, totals);
            EVERY bzc_sum_c(*ss, tid, cnt.data(), nt, base.data());
            delete ss;
        }
        if (s.walk.gather(totals)) {
            std::vector<BzgEntry> ent((size_t)(s.walk.want_ent ? totals[BZG_T_SEL] : 0), BzgEntry{~0ull, ~0ull, ~0ull >> 1, ~0ull});
            ent.shrink_to_fit();
            uint8_t *out = s.walk.want_out ? s.out : nullptr;
            for (uint64_t t = 0; t < tiles; t++) {
                if (cnt[t].bytes == 0) continue;
                select(t);
                EVERY bzc_gather_p3(*sh, tid, g.th[tid], sel[tid]);
                for (uint32_t k = 0; k < 8; k++) EVERY bzg_step_s(sh->g, tid, k);
                CHECK(bzg_bytes(sh->g.s[0][BZF_THREADS - 1]) == cnt[t].bytes, "tile %llu: the gather selects %u bytes, pass two said %u", (ull)t,
                      bzg_bytes(sh->g.s[0][BZF_THREADS - 1]), cnt[t].bytes);
                uint8_t *dst = out ? out + w.w.out_base + base[t].out : nullptr;
                const uint32_t shift = (uint32_t)((uintptr_t)dst & 3u);
                BzgTile x{};
                x.open_start = tile[t].open_start;
                BzgEntry *e = s.walk.want_ent ? ent.data() : nullptr;
                EVERY bzg_gather_p3(sh->g, tid, (uint32_t)t, g.th[tid], x, base[t], w.w, g.tile + tid * BZF_ITEMS, sel[tid].sm, sel[tid].sdm, shift, dst != nullptr, e);
                EVERY bzc_gather_mark(*sh, tid, base[t], sel[tid], e);
                if (dst) EVERY bzg_gather_p4(sh->g, tid, dst, shift, cnt[t].bytes);
            }
            for (size_t k = 0; k < ent.size(); k++) s.ent[w.w.sel_base + k] = ent[k];
        }
        delete sh;
    }
    s.walk.advance(w, bytes, totals);
    return totals[BZC_T_PEND_START];
}

static uint64_t pend_peak_seen, most_windows, over_seen, ctx_seen, groups_seen;
static void ctx_call(const Bytes &text, const Pattern &p, uint32_t B, uint32_t A, const CtxTruth &tr, const std::vector<uint64_t> &blocks, int out_kind, int ent_kind)
{
    const BzfOne m{{}, bzf_pattern(p.pat, p.plen, p.delim)};
    const uint8_t slack = slack_of(p);
    const uint64_t cap = room_of(out_kind, tr.out.size()), max = room_of(ent_kind, tr.ent.size());
    uint8_t *out = out_kind ? (uint8_t *)malloc(cap ? cap : 1) : nullptr;
    std::vector<BzgEntry> ent((size_t)max);
    ent.shrink_to_fit();
    CtxCall s{BzcWalk{}, out, ent_kind ? ent.data() : nullptr, 0};
    if (ent_kind && !max) s.ent = reinterpret_cast<BzgEntry *>(sizeof(BzgEntry));
    s.walk.begin(p.plen, p.invert != 0, B, A, out_kind != 0, cap, ent_kind != 0, max);
    Bytes carry;
    uint64_t pend_truth_peak = 0;
    if (blocks.empty()) {
        const Text d(text.data(), text.size(), slack);
        const uint64_t ts = ctx_run(s, d.p, s.walk.window(0, text.size(), true), text.size(), m);
        carry.assign(d.p + ts, d.p + text.size());
    } else {
        uint64_t at = 0;
        for (uint64_t bytes : blocks) {
            const uint64_t extra = bzg_front_extra(s.walk.carry, BZF_FRONT), front = extra + BZF_FRONT;
            const Text stage(front + bytes, slack);
            memset(stage.p, poison_front, front);
            CHECK(carry.size() == s.walk.carry && front >= carry.size(), "the carry fits in front");
            if (!carry.empty()) memcpy(stage.p + front - carry.size(), carry.data(), carry.size());
            if (bytes) memcpy(stage.p + front, &text[at], bytes);
            at += bytes;
            const uint64_t ts = ctx_run(s, stage.p, s.walk.window(front, bytes, false), bytes, m);
            carry.assign(stage.p + ts, stage.p + front + bytes);
            const uint64_t want = pending_truth(tr, text, p.delim, at - s.walk.held, B, A);
            CHECK(s.walk.npend == want, "pending records behind %llu bytes: %llu, the truth %llu", (ull)at, (ull)s.walk.npend, (ull)want);
            pend_truth_peak = std::max(pend_truth_peak, want);
        }
        CHECK(at == text.size(), "the blocks are the text");
        if (s.walk.held || s.walk.npend) { // GrepSink::finish: the finishing window, over the carry where it lies
            const Text held(carry.data(), carry.size(), slack);
            const uint64_t ts = ctx_run(s, held.p, s.walk.window(s.walk.carry, 0, true), 0, m);
            carry.erase(carry.begin(), carry.begin() + ts);
        }
    }
    CHECK(carry.size() == s.walk.carry && s.walk.held == 0 && s.walk.npend == 0 && s.walk.pend_bytes == 0, "the tail");
    bool copy, entry;
    s.walk.tail_rooms(&copy, &entry);
    const BzgEntry te = s.walk.tail_entry();
    if (copy && !carry.empty()) memcpy(s.out + s.walk.out_bytes, carry.data(), carry.size());
    s.walk.tail_done();
    if (entry) s.ent[s.walk.sel - 1] = te;
    CHECK(s.walk.sel == tr.ent.size() && s.walk.out_bytes == tr.out.size() && s.walk.nrecords() == tr.nrecords,
          "counts: %llu selected of %llu bytes, %llu records; the truth %zu, %zu, %llu", (ull)s.walk.sel, (ull)s.walk.out_bytes, (ull)s.walk.nrecords(), tr.ent.size(),
          tr.out.size(), (ull)tr.nrecords);
    CHECK(s.walk.matched == tr.matched && s.walk.context == tr.context && s.walk.groups == tr.groups, "matched %llu context %llu groups %llu; the truth %llu %llu %llu",
          (ull)s.walk.matched, (ull)s.walk.context, (ull)s.walk.groups, (ull)tr.matched, (ull)tr.context, (ull)tr.groups);
    CHECK(s.walk.pending_peak == pend_truth_peak, "pending_peak %llu, the truth %llu", (ull)s.walk.pending_peak, (ull)pend_truth_peak);
    const bool over = (out_kind && tr.out.size() > cap) || (ent_kind && tr.ent.size() > max);
    CHECK(s.walk.overflow() == over, "BZH_E_CAP exactly when a room that is asked for is too small");
    if (!over) {
        if (out_kind && !tr.out.empty()) CHECK(memcmp(out, tr.out.data(), tr.out.size()) == 0, "the selected bytes");
        for (size_t k = 0; ent_kind && k < tr.ent.size(); k++)
            CHECK(ent[k].record == tr.ent[k].record && ent[k].off == tr.ent[k].off && ent[k].len == tr.ent[k].len && ent[k].out_off == tr.ent[k].out_off,
                  "entry %zu: record %llu off %llu len %llx out_off %llu, the truth %llu %llu %llx %llu", k, (ull)ent[k].record, (ull)ent[k].off, (ull)ent[k].len,
                  (ull)ent[k].out_off, (ull)tr.ent[k].record, (ull)tr.ent[k].off, (ull)tr.ent[k].len, (ull)tr.ent[k].out_off);
    }
    pend_peak_seen = std::max(pend_peak_seen, s.walk.pending_peak), most_windows = std::max(most_windows, s.windows);
    over_seen += over, ctx_seen += tr.context, groups_seen += tr.groups;
    free(out);
}

// ---- texts -------------------------------------------------------------------------------------------------------------------------
static const uint32_t BA[][2] = {{0, 0}, {1, 0}, {0, 1}, {1, 1}, {2, 3}, {16, 16}, {17, 0}, {0, 17}, {5000, 5000}};
static Pattern pattern(uint32_t plen, uint32_t delim, uint32_t invert)
{
    Pattern p{};
    p.plen = plen, p.delim = delim, p.invert = invert;
    for (uint32_t j = 0; j < plen; j++) p.pat[j] = (uint8_t)('a' + (j & 1));
    return p;
}
static void plant(Bytes &text, uint64_t at, const Pattern &p)
{
    if (at + p.plen <= text.size()) memcpy(&text[at], p.pat, p.plen);
}
// letters that never hold the pattern "ab..", one delimiter in `density` bytes (0: none, 1: delimiters only), a hit in one record of `rare`
static Bytes letters(uint64_t n, const Pattern &p, uint64_t density, uint64_t rare)
{
    Bytes t(n);
    for (auto &b : t) b = density && below(density) == 0 ? (uint8_t)p.delim : (uint8_t)('c' + below(2));
    if (rare)
        for (uint64_t at = 0; at + p.plen <= n; at++)
            if (below(rare * (density ? density : 50)) == 0) plant(t, at, p), at += p.plen;
    return t;
}
// records of the given lengths (delimiter included; the last one: `tail` bytes without), the pattern in those listed
static Bytes records(const std::vector<uint64_t> &lens, const std::vector<size_t> &hits, uint64_t tail, bool tail_hit, const Pattern &p)
{
    Bytes t;
    std::vector<uint64_t> starts;
    for (uint64_t l : lens) {
        starts.push_back(t.size());
        t.insert(t.end(), (size_t)l, 'c');
        t.back() = (uint8_t)p.delim;
    }
    const uint64_t ts = t.size();
    t.insert(t.end(), (size_t)tail, 'd');
    for (size_t h : hits)
        if (lens[h] > p.plen) plant(t, starts[h], p);
    if (tail_hit) plant(t, ts, p);
    return t;
}

static uint64_t runs;
static void raw_case(const Bytes &text, const Pattern &p, uint32_t B, uint32_t A)
{
    const CtxTruth tr = naive(text, p, B, A);
    ctx_call(text, p, B, A, tr, {}, 2, 2);
    if (B == 0 && A == 0) { // today's phases on the same input give the same bytes and entries
        GrepTruth plain{tr.out, tr.ent, tr.nrecords};
        const BzfOne m{{}, bzf_pattern(p.pat, p.plen, p.delim)};
        grep_call(text, plain, [&](const BzgWindow &) { return m; }, p.plen, p.invert, slack_of(p), {}, 2, 2);
    }
    runs++;
}
static void every_context(const Bytes &text, const Pattern &p)
{
    for (const auto &ba : BA) raw_case(text, p, ba[0], ba[1]);
}

static void raw_cases()
{
    static const uint64_t ns[] = {0, 1, 15, 16, 17, 4095, 4096, 4097, 8192, 12289};
    static const uint64_t dens[] = {0, 1, 2, 7, 40, 700};
    for (uint64_t n : ns)
        for (uint32_t invert = 0; invert < 2; invert++)
            for (uint64_t density : dens) {
                const Pattern p = pattern(density == 1 ? 1 : 2, '\n', invert);
                Pattern q = p;
                if (density == 1) q.pat[0] = below(2) ? '\n' : 'a'; // delimiters only: every record hit, or none
                every_context(letters(n, q, density, 1 + below(12)), q);
            }
    const Pattern p = pattern(2, '\n', 0), pi = pattern(2, '\n', 1);
    const std::vector<uint64_t> hundred(130, 100);
    // a primary as the last record of a tile / the first record of a tile, the context reaching one and two tiles on / back
    for (uint32_t reach : {1u, 30u, 50u, 90u}) {
        std::vector<uint64_t> lens = hundred;
        lens[0] = 96; // records end at 96 + 100 k: record 40 ends at 4096, record 41 begins the second tile
        const Bytes a = records(lens, {40}, 0, false, p), b = records(lens, {81}, 0, false, p), c = records(lens, {41, 123}, 57, false, p);
        for (const Bytes *t : {&a, &b, &c}) raw_case(*t, p, 0, reach), raw_case(*t, p, reach, 0), raw_case(*t, p, reach, reach), raw_case(*t, pi, 1, reach);
    }
    // a record longer than a tile as context, behind and in front of its primary; and longer than two tiles
    for (uint64_t big : {(uint64_t)6000, (uint64_t)9000}) {
        raw_case(records({10, big, 20, 20}, {0}, 0, false, p), p, 0, 1);
        raw_case(records({10, big, 20, 20}, {2}, 0, false, p), p, 1, 0);
        raw_case(records({10, 20, big, 20, 30}, {1, 3}, 5, false, p), p, 1, 1);
        raw_case(records({10, 20}, {0}, big, false, p), p, 0, 2);
    }
    // two primaries whose contexts overlap, touch, and leave one record between them
    for (size_t gap : {2, 3, 4, 5}) {
        const std::vector<uint64_t> lens(20, 9);
        const Bytes t = records(lens, {5, 5 + gap}, 0, false, p);
        const CtxTruth tr = naive(t, p, 1, 1);
        CHECK(tr.groups == (gap >= 4 ? 2u : 1u), "the planted groups");
        raw_case(t, p, 1, 1), raw_case(t, p, 2, 0), raw_case(t, p, 0, 2);
    }
    // a primary at record 0 with before > 0 and at the last record with after > 0; a primary tail with before > 0; a tail that is
    // after-context; an empty and a non-empty tail
    for (uint64_t tail : {(uint64_t)0, (uint64_t)7, (uint64_t)5000})
        for (int th = 0; th < 2; th++) {
            const std::vector<uint64_t> lens(60, 75);
            for (const auto &ba : BA) {
                raw_case(records(lens, {0}, tail, th != 0, p), p, ba[0], ba[1]);
                raw_case(records(lens, {59}, tail, th != 0, p), p, ba[0], ba[1]);
                raw_case(records(lens, {}, tail, th != 0, p), p, ba[0], ba[1]);
                raw_case(records(lens, {57}, tail, th != 0, pi), pi, ba[0], ba[1]);
            }
        }
    // more tiles than the scans have threads: every scan thread owns several tiles, contexts cross the chunk edges
    for (uint64_t tiles : {(uint64_t)300, (uint64_t)700})
        for (uint32_t invert = 0; invert < 2; invert++) {
            const uint64_t n = tiles * BZF_TILE + 77;
            const Pattern q = pattern(3, '\n', invert);
            Bytes text = letters(n, q, invert ? 3000 : 100, 0);
            for (uint64_t at = 5000; at + 3 < n; at += 70001) plant(text, at, q);
            if (invert) // (inverted: a primary is a record without the pattern; all but a few hold it)
                for (uint64_t at = 0; at + 3 < n; at += 1500)
                    if (at / 200000 % 2 == 0) plant(text, at, q);
            raw_case(text, q, 200, 200), raw_case(text, q, 3, 0), raw_case(text, q, 0, 0);
        }
    CHECK(ctx_seen > runs && groups_seen > runs, "the cases select context records and groups: %llu, %llu", (ull)ctx_seen, (ull)groups_seen);
    printf("raw: %llu calls held (%llu context records, %llu groups)\n", (ull)runs, (ull)ctx_seen, (ull)groups_seen);
}

static void window_cases(uint64_t cases)
{
    const uint64_t over0 = over_seen;
    pend_peak_seen = most_windows = 0;
    uint64_t tail_only = 0, bare = 0, b_above = 0;
    for (uint64_t c = 0; c < cases; c++) {
        const uint32_t nb = 1 + (uint32_t)below(7);
        std::vector<uint64_t> blocks, wins;
        uint64_t n = 0;
        for (uint32_t k = 0; k < nb; k++) blocks.push_back(1 + below(below(4) ? 600 : 9000)), n += blocks.back();
        for (uint32_t k = 0; k < nb;) {
            uint64_t sum = 0;
            const uint32_t take = 1 + (uint32_t)below(4);
            for (uint32_t j = 0; j < take && k < nb; j++, k++) sum += blocks[k];
            wins.push_back(sum);
        }
        static const uint32_t plens[] = {1, 2, 3, 4, 5, 16, 17, 255, 256};
        const uint32_t delim = below(4) ? '\n' : (uint32_t)(0x80 + below(0x60));
        Pattern p = pattern(plens[below(9)], delim, (uint32_t)below(2));
        if (below(4) == 0) p.pat[0] = (uint8_t)delim;             // a pattern that begins with the delimiter,
        if (below(4) == 0) p.pat[p.plen - 1] = (uint8_t)delim;    // ... and one that ends with it
        static const uint64_t dens[] = {0, 2, 9, 40, 700};
        const uint64_t density = dens[below(5)];
        Bytes text = letters(n, p, density, p.invert ? 0 : 1 + below(30));
        if (p.invert && density) // few records without the pattern
            for (uint64_t at = 0; at + p.plen <= n; at += 1 + below(2 * density)) plant(text, at, p);
        // a window without any delimiter between two with
        if (wins.size() >= 3 && below(3) == 0) {
            const size_t k = 1 + below(wins.size() - 2);
            uint64_t lo = 0;
            for (size_t j = 0; j < k; j++) lo += wins[j];
            for (uint64_t j = lo; j < lo + wins[k]; j++)
                if (text[j] == delim) text[j] = 'd';
            bare++;
        }
        bool only_tail = false;
        if (below(8) == 0 && !p.invert && p.pat[0] != delim && p.pat[p.plen - 1] != delim) { // the only primary is the tail
            for (auto &b : text) b = b == delim ? b : 'd';
            if (n > p.plen + 1) {
                text[n - p.plen - 1] = (uint8_t)delim;
                plant(text, n - p.plen, p);
                only_tail = true, tail_only++;
            }
        }
        const uint32_t *ba = BA[below(9)];
        uint32_t B = ba[0], A = ba[1];
        if (below(5) == 0) B = 1 + (uint32_t)below(8), A = (uint32_t)below(4);
        if (below(30) == 0) B = A = 0xFFFFFFFFu;
        const CtxTruth tr = naive(text, p, B, A);
        if (only_tail) CHECK(tr.matched == 1 && tr.prim.back(), "the planted tail");
        b_above += B > tr.nrecords / wins.size();
        ctx_call(text, p, B, A, tr, wins, (int)below(5), (int)below(5));
        ctx_call(text, p, B, A, tr, wins, 2, 2); // (and with the exact rooms)
    }
    const uint64_t over = over_seen - over0;
    CHECK(pend_peak_seen >= 16 && most_windows >= 5 && over > cases / 20 && tail_only > cases / 40 && bare > cases / 20 && b_above > cases / 10,
          "the cases reach the edges: pending %llu, windows %llu, too small %llu, tail only %llu, bare windows %llu, before above a window's records %llu", (ull)pend_peak_seen,
          (ull)most_windows, (ull)over, (ull)tail_only, (ull)bare, (ull)b_above);
    printf("windows: %llu cases held (most pending %llu, most windows %llu, %llu with too little room)\n", (ull)cases, (ull)pend_peak_seen, (ull)most_windows, (ull)over);
}

int main(int argc, char **argv)
{
    rng_state = (argc > 1 ? strtoull(argv[1], nullptr, 10) : 1) * 0x9E3779B97F4A7C15ull + 1;
    const uint64_t cases = argc > 2 ? strtoull(argv[2], nullptr, 10) : 200;
    static_assert(sizeof(bzh_grep_entry) == sizeof(BzgEntry) && BZC_LEN_CONTEXT == BZH_GREP_LEN_CONTEXT, "the entry and its context bit");
    raw_cases();
    window_cases(cases);
    return 0;
}
