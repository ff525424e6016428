// grep_many_host.cpp -- the grep over many texts in one buffer without a device: the virtual-tile plan of
// banzai_amd/csrc/grep_many_plan.h and the phases of grep_many_core.h / grep_core.h, thread by thread and tile by tile in the layout
// of grep_many_tiles and grep_many_scan (banzai_amd/csrc/grep_many.hip), against a naive split-and-find of every segment alone.
// Every buffer is allocated at its exact size, so a read or a store outside it is a sanitizer report.
// usage: grep_many_host SEED
#define HOST_NAME "grep_many_host"
#include "scan_host.h"

#include "../../banzai_amd/csrc/grep_many_plan.h"

typedef std::vector<uint64_t> Words;

struct ManyTruth {
    Bytes out;
    std::vector<BzgEntry> ent;
    Words totals; // [segments][BZGM_TOTALS]
};

// every segment alone: cut at the delimiter, a non-empty tail is the last record; a record is hit when the pattern starts in it
// and ends inside the segment
static ManyTruth truth_of(const Bytes &buf, const Words &offs, const Words &lens, const Bytes &pat, uint8_t delim, bool invert)
{
    ManyTruth tr;
    tr.totals.assign(offs.size() * BZGM_TOTALS, 0);
    for (size_t k = 0; k < offs.size(); k++) {
        const uint8_t *t = buf.data() + offs[k];
        const uint64_t n = lens[k];
        uint64_t rec = 0, start = 0;
        while (start < n) {
            uint64_t end = start;
            while (end < n && t[end] != delim) end++;
            if (end < n) end++; // (the delimiter belongs to the record it ends)
            bool hit = false;
            for (uint64_t p = start; p < end && !hit; p++) hit = p + pat.size() <= n && memcmp(t + p, pat.data(), pat.size()) == 0;
            if (hit != invert) {
                tr.ent.push_back(BzgEntry{rec, start, end - start, tr.out.size()});
                tr.out.insert(tr.out.end(), t + start, t + end);
                tr.totals[k * BZGM_TOTALS + BZGM_T_SEL]++;
                tr.totals[k * BZGM_TOTALS + BZGM_T_BYTES] += end - start;
            }
            rec++, start = end;
        }
        tr.totals[k * BZGM_TOTALS + BZGM_T_RECORDS] = rec;
    }
    return tr;
}

// the front of grep_many_tiles for virtual tile v: the row, the segment's window, the rebound matcher, the masks with the closing
// bit, the forward scan
static void many_front(const uint8_t *d, const BzgmPlan &plan, uint32_t v, const BzfOne &m0, uint32_t invert, Group<BzfOne> &g, BzgWindow *w)
{
    const BzgmRow r = plan.row[v];
    const BzgmSeg s = plan.seg[r.seg];
    BzfOne m = m0;
    *w = bzgm_window(s, m.p.plen, invert);
    bzgm_rebind(m, s.lo, s.hi);
    g.stage(m, d, w->n, r.tile);
    EVERY {
        const uint64_t p0 = (uint64_t)r.tile * BZF_TILE + tid * BZF_ITEMS;
        bzg_masks(g.th[tid], *w, p0, g.own[tid], m.delim(), m.match16(g.own[tid], tid, p0, g.tile, *g.msh, bzg_starts(*w, p0)));
        bzgm_close(g.th[tid], *w, p0);
        bzg_local(g.th[tid], w->invert);
    }
    EVERY bzg_count_p0(*g.sh, tid, g.th[tid]);
    for (uint32_t k = 0; k < 8; k++) EVERY bzg_step_f(*g.sh, tid, k);
}

static uint64_t runs = 0;

// GrepSink::raw_many over buf (n bytes, the segments inside) against the truth; rooms by kind (scan_host.h: room_of)
static void many_call(const Bytes &buf, const Words &offs, const Words &lens, const Bytes &pat, uint8_t delim, uint32_t invert, int out_kind, int ent_kind,
                      uint64_t *shared = nullptr)
{
    runs++;
    size_t bad = 0;
    CHECK(bzgm_check(offs.data(), lens.data(), offs.size(), buf.size(), &bad) == nullptr, "the segments of a case are well formed (%zu)", bad);
    const ManyTruth tr = truth_of(buf, offs, lens, pat, delim, invert != 0);
    const Text d(buf.data(), buf.size(), 0xEE);
    BzgmPlan plan;
    CHECK(plan.build(offs.data(), lens.data(), offs.size()), "the rows fit one launch");
    if (shared) *shared = plan.shared;
    // the plan: one row per (segment, tile it meets), in segment order
    {
        uint64_t v = 0;
        for (size_t k = 0; k < offs.size(); k++) {
            const BzgmSeg &s = plan.seg[k];
            CHECK(s.lo == offs[k] && s.hi == offs[k] + lens[k], "segment %zu", k);
            if (!lens[k]) {
                CHECK(s.rows == 0, "an empty segment owns no tile");
                continue;
            }
            CHECK(s.first == v && s.rows == (s.hi - 1) / BZF_TILE - s.lo / BZF_TILE + 1, "segment %zu owns rows [%u, +%u)", k, s.first, s.rows);
            for (uint32_t j = 0; j < s.rows; j++, v++) CHECK(plan.row[v].seg == k && plan.row[v].tile == s.lo / BZF_TILE + j, "row %llu", (ull)v);
        }
        CHECK(v == plan.rows && plan.row.size() == v, "the rows");
    }
    const uint32_t rows = (uint32_t)plan.rows, segs = (uint32_t)offs.size();
    const BzfOne m0{{}, bzf_pattern(pat.data(), (uint32_t)pat.size(), delim)};
    const uint64_t cap = room_of(out_kind, tr.out.size()), max = room_of(ent_kind, tr.ent.size());
    uint8_t *out = out_kind ? (uint8_t *)malloc(cap ? cap : 1) : nullptr;
    std::vector<BzgEntry> ent((size_t)max, BzgEntry{~0ull, ~0ull, ~0ull, ~0ull});
    ent.shrink_to_fit();
    Words totals(BZG_TOTALS + (size_t)segs * BZGM_TOTALS, 0);
    totals.shrink_to_fit();
    bool fits = true;
    if (rows) {
        BzgmSeg *seg = exact(plan.seg.data(), plan.seg.size());
        BzgmRow *row = exact(plan.row.data(), plan.row.size());
        std::vector<BzgTile> tile(rows);
        std::vector<BzgBase> base(rows);
        tile.shrink_to_fit(), base.shrink_to_fit();
        Group<BzfOne> g;
        BzgWindow w;
        for (uint32_t v = 0; v < rows; v++) {
            many_front(d.p, plan, v, m0, invert, g, &w);
            EVERY bzg_count_p1(*g.sh, tid, g.th[tid], w.invert);
            for (uint32_t k = 0; k < 8; k++) EVERY bzg_step_s(*g.sh, tid, k);
            bzg_count_p2(*g.sh, tile[v]);
        }
        { // grep_many_scan
            BzgScanShared *sh = new BzgScanShared;
            memset((void *)sh, 0xAA, sizeof *sh);
            const BzgManyTexts texts{row, seg};
            BzgWindow sw{};
            sw.invert = invert;
            EVERY bzg_scan_a(*sh, tid, tile.data(), rows, texts);
            bzg_scan_b(*sh, sw, totals.data());
            EVERY bzg_scan_c(*sh, tid, tile.data(), rows, sw, texts);
            bzg_scan_d(*sh);
            EVERY bzg_scan_e(*sh, tid, tile.data(), rows, sw, texts);
            bzg_scan_f(*sh, totals.data());
            EVERY bzg_scan_g(*sh, tid, tile.data(), rows, base.data());
            for (uint32_t k = 0; k < segs; k++) bzgm_totals(seg, k, base.data(), rows, totals.data(), totals.data() + BZG_TOTALS);
            delete sh;
        }
        const BzgmRooms rooms{out_kind != 0, ent_kind != 0, cap, max};
        fits = rooms.fits(totals[BZG_T_BYTES], totals[BZG_T_SEL]);
        if (rooms.gather(totals[BZG_T_BYTES], totals[BZG_T_SEL])) {
            for (uint32_t v = 0; v < rows; v++) {
                const BzgTile &x = tile[v];
                if (x.bytes == 0) continue;
                const BzgmRow r = row[v];
                const BzgBase b = bzgm_base(base.data(), v, seg[r.seg]);
                many_front(d.p, plan, v, m0, invert, g, &w);
                bool sel_first[BZF_THREADS];
                uint32_t sm[BZF_THREADS], sdm[BZF_THREADS];
                EVERY bzg_gather_p1(*g.sh, tid, g.th[tid], x, w.invert, &sel_first[tid]);
                for (uint32_t k = 0; k < 8; k++) EVERY bzg_step_b(*g.sh, tid, k);
                EVERY bzg_gather_p2(*g.sh, tid, g.th[tid], x, sel_first[tid], &sm[tid], &sdm[tid]);
                for (uint32_t k = 0; k < 8; k++) EVERY bzg_step_s(*g.sh, tid, k);
                CHECK(bzg_bytes(g.sh->s[0][BZF_THREADS - 1]) == x.bytes, "row %u: the gather selects %u bytes, the scan said %u", v, bzg_bytes(g.sh->s[0][BZF_THREADS - 1]), x.bytes);
                uint8_t *dst = out ? out + b.out : nullptr;
                const uint32_t shift = (uint32_t)((uintptr_t)dst & 3u);
                EVERY bzg_gather_p3(*g.sh, tid, r.tile, g.th[tid], x, b, w, g.tile + tid * BZF_ITEMS, sm[tid], sdm[tid], shift, dst != nullptr, ent_kind ? ent.data() : nullptr);
                if (dst) EVERY bzg_gather_p4(*g.sh, tid, dst, shift, x.bytes);
            }
        }
        free(seg), free(row);
    }
    CHECK(totals[BZG_T_SEL] == tr.ent.size() && totals[BZG_T_BYTES] == tr.out.size(), "the call's counts: %llu selected of %llu bytes, the truth %zu of %zu",
          (ull)totals[BZG_T_SEL], (ull)totals[BZG_T_BYTES], tr.ent.size(), tr.out.size());
    for (size_t j = 0; j < (size_t)segs * BZGM_TOTALS; j++)
        CHECK(totals[BZG_TOTALS + j] == tr.totals[j], "segment %zu, total %zu: %llu, the truth %llu", j / BZGM_TOTALS, j % BZGM_TOTALS, (ull)totals[BZG_TOTALS + j], (ull)tr.totals[j]);
    const bool over = (out_kind && tr.out.size() > cap) || (ent_kind && tr.ent.size() > max);
    CHECK(fits == !over, "BZH_E_CAP exactly when a room that is asked for is too small");
    if (!over) {
        if (out_kind && !tr.out.empty()) CHECK(memcmp(out, tr.out.data(), tr.out.size()) == 0, "the selected bytes");
        for (size_t k = 0; ent_kind && k < tr.ent.size(); k++)
            CHECK(ent[k].record == tr.ent[k].record && ent[k].off == tr.ent[k].off && ent[k].len == tr.ent[k].len && ent[k].out_off == tr.ent[k].out_off,
                  "entry %zu: record %llu off %llu len %llu out_off %llu, the truth %llu %llu %llu %llu", k, (ull)ent[k].record, (ull)ent[k].off, (ull)ent[k].len,
                  (ull)ent[k].out_off, (ull)tr.ent[k].record, (ull)tr.ent[k].off, (ull)tr.ent[k].len, (ull)tr.ent[k].out_off);
    }
    free(out);
}

// the three room shapes of the issue beside the plain call: at the need, one below (either room), not asked for
static void many_rooms(const Bytes &buf, const Words &offs, const Words &lens, const Bytes &pat, uint8_t delim, uint32_t invert)
{
    static const int kinds[][2] = {{2, 2}, {3, 2}, {2, 3}, {0, 0}, {2, 0}, {0, 2}};
    for (const auto &k : kinds) many_call(buf, offs, lens, pat, delim, invert, k[0], k[1]);
}

static Bytes pattern_of(uint32_t plen)
{
    Bytes p(plen);
    for (auto &b : p) b = (uint8_t)('a' + below(3));
    p[below(plen)] = 'q'; // (no text byte is 'q' unless planted: a hit is a planted one, or made of them)
    return p;
}
// text over a small alphabet with a delimiter every `every` bytes on average (0: none)
static void fill(Bytes &buf, uint64_t lo, uint64_t hi, uint8_t delim, uint32_t every)
{
    for (uint64_t p = lo; p < hi; p++) buf[p] = every && below(every) == 0 ? delim : (uint8_t)('a' + below(3));
}
static void plant(Bytes &buf, uint64_t at, const Bytes &pat)
{
    if (at + pat.size() <= buf.size()) memcpy(&buf[at], pat.data(), pat.size());
}

int main(int argc, char **argv)
{
    rng_state = argc > 1 ? strtoull(argv[1], nullptr, 10) * 0x9E3779B97F4A7C15ull + 1 : 1;
    const uint8_t delim = '\n';
    static const uint32_t plens[] = {1, 2, 16, 17, 256};
    static const uint64_t seglens[] = {0, 1, 15, 16, 17, 4095, 4096, 4097, 8193};

    // (1) every segment length, the first start at every residue modulo 16 (the later ones fall where the lengths put them, with
    // a gap now and then), the pattern planted inside segments and across walls, every plen, both senses
    for (uint32_t res = 0; res < 16; res++)
        for (uint32_t plen : plens)
            for (uint32_t invert = 0; invert < 2; invert++) {
                const Bytes pat = pattern_of(plen);
                Words offs, lens;
                uint64_t at = res;
                std::vector<size_t> order;
                for (size_t j = 0; j < sizeof seglens / sizeof *seglens; j++) order.push_back(j);
                for (size_t j = order.size(); j > 1; j--) std::swap(order[j - 1], order[below(j)]);
                for (size_t j : order) {
                    offs.push_back(at), lens.push_back(seglens[j]);
                    at += seglens[j] + (below(3) == 0 ? below(40) : 0);
                }
                Bytes buf((size_t)at);
                fill(buf, 0, at, delim, 1 + (uint32_t)below(200));
                for (size_t k = 0; k < offs.size(); k++) { // inside, at both ends, and across the wall behind the segment
                    if (lens[k] >= plen) plant(buf, offs[k] + below(lens[k] - plen + 1), pat), plant(buf, offs[k], pat);
                    if (below(2)) plant(buf, offs[k] + lens[k] - std::min<uint64_t>(lens[k], below(plen + 1)), pat);
                }
                if (res % 4 == 0 && plen == 17) many_rooms(buf, offs, lens, pat, delim, invert);
                else many_call(buf, offs, lens, pat, delim, invert, 2, 2);
            }
    printf("shapes: %llu calls held\n", (ull)runs);

    for (uint32_t plen : plens)
        for (uint32_t invert = 0; invert < 2; invert++) {
            const Bytes pat = pattern_of(plen);
            { // (2) a segment ends on a tile's last byte, the next starts on the next tile's first
                Bytes buf(2 * BZF_TILE + 500);
                fill(buf, 0, buf.size(), delim, 50);
                plant(buf, BZF_TILE - plen, pat), plant(buf, BZF_TILE, pat), plant(buf, BZF_TILE - plen / 2 - 1, pat);
                uint64_t shared = ~0ull;
                many_call(buf, Words{100, BZF_TILE}, Words{BZF_TILE - 100, BZF_TILE + 400}, pat, delim, invert, 2, 2, &shared);
                CHECK(shared == 0, "no tile is shared when a wall stands on a tile edge");
            }
            { // (3) 40 segments of 100 bytes in one tile
                Bytes buf(4000);
                fill(buf, 0, buf.size(), delim, 30);
                Words offs, lens;
                for (uint64_t k = 0; k < 40; k++) {
                    offs.push_back(100 * k), lens.push_back(100);
                    if (plen <= 100 && below(2)) plant(buf, 100 * k + below(100 - plen + 1), pat);
                    if (below(3) == 0) plant(buf, 100 * k + 100 - std::min<uint32_t>(plen, 100) / 2, pat);
                }
                uint64_t shared = 0;
                many_call(buf, offs, lens, pat, delim, invert, 2, 2, &shared);
                CHECK(shared == 1, "one tile is shared by the 40 segments");
            }
            { // (4) a gap between two segments, filled with the needle
                Bytes buf(3000 + 4 * plen);
                fill(buf, 0, buf.size(), delim, 40);
                const uint64_t g0 = 1000, g1 = g0 + 4 * plen;
                for (uint64_t p = g0; p + plen <= g1; p += plen) plant(buf, p, pat);
                many_call(buf, Words{3, g1}, Words{g0 - 3, buf.size() - g1}, pat, delim, invert, 2, 2);
            }
            { // (5) a segment of delimiters only, between two of text; (7) a last byte that is and is not the delimiter
                Bytes buf(900);
                fill(buf, 0, buf.size(), delim, 25);
                memset(&buf[300], delim, 300);
                buf[299] = delim, buf[899] = 'a';
                if (plen <= 250) plant(buf, 20, pat), plant(buf, 899 - plen, pat);
                many_call(buf, Words{0, 300, 600}, Words{300, 300, 300}, pat, delim, invert, 2, 2);
                buf[299] = 'b', buf[899] = delim;
                many_call(buf, Words{0, 300, 600}, Words{300, 300, 300}, pat, delim, invert, 2, 2);
            }
            // (6) a segment without a delimiter over three tiles, its only hit in the first, the middle and the last tile
            for (uint32_t where = 0; where < 3; where++) {
                const uint64_t lo = 700, len = 2 * BZF_TILE + 900;
                Bytes buf(lo + len + 300);
                fill(buf, 0, buf.size(), delim, 0);
                buf[lo - 1] = delim, buf[lo + len] = delim;
                plant(buf, where == 0 ? lo + 5 : where == 1 ? BZF_TILE + 2000 : lo + len - plen, pat);
                many_call(buf, Words{0, lo, lo + len}, Words{lo, len, 300}, pat, delim, invert, 2, 2);
            }
            // (8) the needle cut at every point across a wall: no hit, whatever stands beside the wall
            for (uint32_t cut = 1; cut < plen; cut++) {
                const uint64_t wall = 4090 + below(20);
                Bytes buf(wall + 600);
                memset(buf.data(), 'x', buf.size());
                for (uint64_t p = 37; p < buf.size(); p += 61) buf[p] = delim;
                plant(buf, wall - cut, pat);
                many_call(buf, Words{wall > 500 ? wall - 500 : 0, wall}, Words{wall > 500 ? 500 : wall, 600}, pat, delim, invert, 2, 2);
                if (!invert) {
                    const ManyTruth tr = truth_of(buf, Words{wall - 500, wall}, Words{500, 600}, pat, delim, false);
                    CHECK(tr.ent.empty(), "a needle cut at %u by a wall is no hit", cut);
                }
            }
        }
    // no segment at all, and only empty ones
    many_call(Bytes(10, 'a'), Words{}, Words{}, Bytes{'a'}, delim, 0, 2, 2);
    many_call(Bytes(10, 'a'), Words{0, 5, 10}, Words{0, 0, 0}, Bytes{'a'}, delim, 1, 2, 2);
    // what the plan refuses
    {
        size_t bad = 99;
        const Words o1{0, 5}, l1{6, 2}, o2{8, 2}, l2{2, 2}, o3{0, 9}, l3{2, 2};
        CHECK(bzgm_check(o1.data(), l1.data(), 2, 100, &bad) && bad == 1, "overlapping segments are refused");
        CHECK(bzgm_check(o2.data(), l2.data(), 2, 100, &bad) && bad == 1, "descending segments are refused");
        CHECK(bzgm_check(o3.data(), l3.data(), 2, 10, &bad) && bad == 1, "a segment past the end is refused");
    }
    { // more virtual tiles than one launch takes: the rows are counted, no table is built
        BzgmPlan big;
        const Words o{5, (1ull << 44) + 9}, l{1ull << 44, 3};
        CHECK(!big.build(o.data(), l.data(), 2), "2^32 virtual tiles are refused");
        CHECK(big.rows == (1ull << 32) + 2 && big.rows > BZGM_MAX_ROWS && big.row.empty() && big.nonempty == 2, "the rows beyond one launch: %llu", (ull)big.rows);
        const Words o2{0}, l2{(uint64_t)BZGM_MAX_ROWS * BZF_TILE + 1};
        CHECK(!big.build(o2.data(), l2.data(), 1) && big.rows == BZGM_MAX_ROWS + 1, "one row above the limit is refused");
    }
    printf("walls: %llu calls held\n", (ull)runs);
    return 0;
}
