// records_host.cpp -- the host arithmetic of reads by record number (banzai_amd/csrc/decode_records_plan.h: the table check, the
// clipping, bzq_spans, which is bzh_record_spans, and the walk of bzh_decode_records over its batches -- the queries it sends to
// unrle_select and the pieces it has the blocks emitted by) against brute force per output byte, built with
// g++ -fsanitize=address,undefined.  The device is played by the brute force itself: a synthetic index, a flag a byte that says
// whether it is a delimiter, tiles that share a block's bytes at random.  The decoded bytes are their own positions, so a byte
// in the wrong place shows as a wrong value.
//
//   records_host <seed> <cases>     exit status 0: everything held for <cases> seeded cases (and the fixed ones)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <vector>

#include "../../include/bzhip.h"
#include "../../banzai_amd/csrc/decode_records_plan.h"

static uint64_t rng_state;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}
static uint64_t below(uint64_t n) { return n ? rnd() % n : 0; }

#define CHECK(cond, ...)                                   \
    do {                                                   \
        if (!(cond)) {                                     \
            fprintf(stderr, "records_host: %s: ", #cond);  \
            fprintf(stderr, __VA_ARGS__);                  \
            fprintf(stderr, "\n");                         \
            exit(1);                                       \
        }                                                  \
    } while (0)

static std::vector<bzh_index_entry> make_index(const std::vector<uint32_t> &sizes)
{
    std::vector<bzh_index_entry> idx(sizes.size());
    uint64_t bit = 32, off = 0;
    for (size_t k = 0; k < sizes.size(); k++) {
        const uint64_t bits = 174 + below(900);
        idx[k] = bzh_index_entry{bit, bit + bits, off, sizes[k], (uint32_t)rnd(), (uint32_t)(k / 3), 1 + (uint32_t)below(9)};
        bit += bits + (below(3) ? 0 : 80 + below(200));
        off += sizes[k];
    }
    return idx;
}

// The tiles of a block of `size` output bytes: some put out nothing, the others share the bytes at random.
static void make_tiles(uint32_t size, uint32_t tn, uint32_t *tout)
{
    for (uint32_t t = 0; t < tn; t++) tout[t] = 0;
    for (uint32_t left = size; left;) {
        const uint32_t t = (uint32_t)below(tn), take = 1 + (uint32_t)below(left);
        tout[t] += take;
        left -= take;
    }
}

static uint64_t sat_add(uint64_t a, uint64_t b) { return a + b < a ? ~0ull : a + b; }

// isd[p]: output byte p is a delimiter
static void records_case(const std::vector<uint32_t> &sizes, const std::vector<uint8_t> &isd, const std::vector<bzh_range> &ranges, uint32_t Bmax,
                         uint32_t Tn, bool ascending)
{
    const std::vector<bzh_index_entry> idx = make_index(sizes);
    const size_t count = idx.size(), nr = ranges.size();
    const uint64_t total = isd.size();
    std::vector<uint64_t> p; // p[k - 1] = the position of delimiter k
    std::vector<uint32_t> entry_of(total);
    std::vector<uint64_t> rec_cum(count + 1, 0);
    for (size_t k = 0; k < count; k++) {
        rec_cum[k] = p.size();
        for (uint32_t j = 0; j < sizes[k]; j++) {
            entry_of[idx[k].out_off + j] = (uint32_t)k;
            if (isd[idx[k].out_off + j]) p.push_back(idx[k].out_off + j);
        }
    }
    const uint64_t D = p.size();
    rec_cum[count] = D;
    size_t bad = 0;
    CHECK(bzq_table_check(idx.data(), count, rec_cum.data(), &bad) == nullptr, "a true table is refused at entry %zu", bad);
    auto s_of = [&](uint64_t k) { return k == 0 ? 0 : k <= D ? p[k - 1] + 1 : total; }; // the first byte of record k

    // brute force: every range's bytes, and the entries it touches
    std::vector<uint64_t> want, want_offs(nr), want_lens(nr);
    std::set<uint32_t> want_touched;
    for (size_t r = 0; r < nr; r++) {
        const uint64_t a = ranges[r].off < D + 1 ? ranges[r].off : D + 1;
        uint64_t b = sat_add(ranges[r].off, ranges[r].len);
        b = b < D + 1 ? b : D + 1;
        if (b < a) b = a;
        want_offs[r] = want.size();
        for (uint64_t q = s_of(a); a < b && q < s_of(b); q++) want.push_back(q);
        want_lens[r] = want.size() - want_offs[r];
        if (a == b || count == 0) continue;
        const uint32_t first = a == 0 ? 0 : entry_of[p[a - 1]], last = b <= D ? entry_of[p[b - 1]] : (uint32_t)count - 1;
        for (uint32_t e = first; e <= last; e++) want_touched.insert(e);
    }
    std::vector<uint32_t> touched;
    uint64_t lo, hi;
    bzq_spans(idx.data(), count, rec_cum.data(), ranges.data(), nr, touched, &lo, &hi);
    CHECK(touched.size() == want_touched.size() && std::equal(touched.begin(), touched.end(), want_touched.begin()), "the touched entries differ");
    CHECK(lo == (touched.empty() ? 0 : idx[touched.front()].bit_pos / 8) && hi == (touched.empty() ? 0 : (idx[touched.back()].end_bit + 7) / 8),
          "the hull [%llu, %llu)", (unsigned long long)lo, (unsigned long long)hi);

    BzqWalk<bzh_index_entry, bzh_range> walk;
    const bool ok = walk.start(idx.data(), count, rec_cum.data(), ranges.data(), nr, &bad);
    if (!ascending) { // the brute force of the rule: some range begins in front of the end of the one before it
        size_t first_bad = nr;
        uint64_t end = 0;
        for (size_t r = 0; r < nr && first_bad == nr; r++) {
            const uint64_t a = ranges[r].off < D + 1 ? ranges[r].off : D + 1;
            uint64_t b = sat_add(ranges[r].off, ranges[r].len);
            b = b < D + 1 ? b : D + 1;
            if (a < end) first_bad = r;
            end = b;
        }
        CHECK(ok == (first_bad == nr) && (ok || bad == first_bad), "a list that does not ascend: range %zu named, %zu expected", bad, first_bad);
        if (!ok) return;
    }
    CHECK(ok, "an ascending list is refused at range %zu", bad);

    // the batches: the device's answers come from the flags
    std::vector<uint64_t> out(want.size(), ~0ull);
    std::vector<uint32_t> written(want.size(), 0);
    std::vector<size_t> out_offs(nr ? nr : 1, 12345), out_lens(nr ? nr : 1, 12345);
    std::vector<BzqQuery> q;
    std::vector<size_t> pfirst;
    std::vector<PieceRef> pc;
    std::set<uint32_t> emitted_from;
    for (size_t t0 = 0; t0 < touched.size();) {
        const uint32_t B = (uint32_t)std::min<size_t>(Bmax, touched.size() - t0);
        const uint32_t *ent = touched.data() + t0;
        std::vector<uint32_t> tout((size_t)B * Tn), toff((size_t)B * Tn), tcount((size_t)B * Tn, 0), ntiles(B);
        for (uint32_t k = 0; k < B; k++) {
            ntiles[k] = 1 + (uint32_t)below(Tn);
            make_tiles(sizes[ent[k]], ntiles[k], tout.data() + (size_t)k * Tn);
            uint32_t at = 0;
            for (uint32_t t = 0; t < ntiles[k]; t++) {
                toff[(size_t)k * Tn + t] = at;
                for (uint32_t j = 0; j < tout[(size_t)k * Tn + t]; j++) tcount[(size_t)k * Tn + t] += isd[idx[ent[k]].out_off + at + j];
                at += tout[(size_t)k * Tn + t];
            }
        }
        CHECK(walk.queries(ent, B, tcount.data(), Tn, ntiles.data(), q, &bad), "true tile counts are refused at entry %zu", bad);
        std::vector<uint32_t> pos(q.size() ? q.size() : 1, BZQ_NONE);
        for (size_t i = 0; i < q.size(); i++) { // unrle_select, by brute force: the k-th delimiter of the tile
            CHECK(q[i].slot < B && q[i].tile < ntiles[q[i].slot], "query %zu names slot %u tile %u", i, q[i].slot, q[i].tile);
            const size_t cell = (size_t)q[i].slot * Tn + q[i].tile;
            CHECK(q[i].k >= 1 && q[i].k <= tcount[cell], "query %zu asks for delimiter %u of %u", i, q[i].k, tcount[cell]);
            uint32_t seen = 0;
            for (uint32_t j = 0; j < tout[cell]; j++)
                if (isd[idx[ent[q[i].slot]].out_off + toff[cell] + j] && ++seen == q[i].k) {
                    pos[i] = toff[cell] + j;
                    break;
                }
        }
        uint64_t batch_end = 0;
        CHECK(walk.place(ent, B, pos.data(), out_offs.data(), out_lens.data(), pfirst, pc, &batch_end, &bad), "true positions are refused at entry %zu", bad);
        CHECK(pfirst.size() == (size_t)B + 1 && pfirst[0] == 0 && pfirst[B] == pc.size(), "the piece table of the batch");
        uint64_t seen_end = 0;
        for (uint32_t k = 0; k < B; k++)
            for (size_t i = pfirst[k]; i < pfirst[k + 1]; i++) {
                const PieceRef &c = pc[i];
                CHECK(c.lo < c.hi && c.hi <= sizes[ent[k]], "piece [%u, %u) of a block of %u bytes", c.lo, c.hi, sizes[ent[k]]);
                CHECK(c.base + (c.hi - c.lo) <= want.size(), "a piece ends at %llu of %zu output bytes", (unsigned long long)(c.base + c.hi - c.lo), want.size());
                for (uint32_t j = c.lo; j < c.hi; j++) {
                    out[c.base + (j - c.lo)] = idx[ent[k]].out_off + j;
                    written[c.base + (j - c.lo)]++;
                }
                seen_end = std::max<uint64_t>(seen_end, c.base + (c.hi - c.lo));
                emitted_from.insert(ent[k]);
            }
        CHECK(seen_end == batch_end, "batch_end %llu, the pieces end at %llu", (unsigned long long)batch_end, (unsigned long long)seen_end);
        t0 += B;
    }
    walk.finish(out_offs.data(), out_lens.data());
    CHECK(walk.run_off == want.size(), "%llu bytes placed, %zu wanted", (unsigned long long)walk.run_off, want.size());
    for (size_t r = 0; r < nr; r++)
        CHECK(out_offs[r] == want_offs[r] && out_lens[r] == want_lens[r], "range %zu: [%zu, +%zu), wanted [%llu, +%llu)", r, out_offs[r], out_lens[r],
              (unsigned long long)want_offs[r], (unsigned long long)want_lens[r]);
    for (size_t i = 0; i < want.size(); i++)
        CHECK(written[i] == 1 && out[i] == want[i], "output byte %zu: written %u times, holds %llu, wanted %llu", i, written[i],
              (unsigned long long)out[i], (unsigned long long)want[i]);
    for (uint32_t e : emitted_from) CHECK(want_touched.count(e), "bytes of entry %u, which is not touched", e);
}

static void refused_tables()
{
    const std::vector<uint32_t> sizes = {3, 1, 4};
    const std::vector<bzh_index_entry> idx = make_index(sizes);
    size_t bad = 0;
    const uint64_t good[4] = {0, 3, 3, 7}, first[4] = {1, 3, 3, 7}, desc[4] = {0, 3, 2, 7}, fat[4] = {0, 3, 5, 7};
    CHECK(!bzq_table_check(idx.data(), 3, good, &bad), "every byte a delimiter is a table");
    CHECK(bzq_table_check(idx.data(), 3, first, &bad), "rec_cum[0] != 0");
    CHECK(bzq_table_check(idx.data(), 3, desc, &bad) && bad == 1, "a descending table, entry %zu", bad);
    CHECK(bzq_table_check(idx.data(), 3, fat, &bad) && bad == 1, "more delimiters than bytes, entry %zu", bad);
    // tile counts that do not sum to the table's are refused by the walk, the entry named
    BzqWalk<bzh_index_entry, bzh_range> walk;
    const bzh_range all = {0, ~0ull};
    CHECK(walk.start(idx.data(), 3, good, &all, 1, &bad), "one range");
    const uint32_t ent[3] = {0, 1, 2}, tcount[3] = {3, 1, 3}, ntiles[3] = {1, 1, 1};
    std::vector<BzqQuery> q;
    CHECK(!walk.queries(ent, 3, tcount, 1, ntiles, q, &bad) && bad == 1, "a count moved to the neighbour, entry %zu", bad);
}

int main(int argc, char **argv)
{
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int cases = argc > 2 ? atoi(argv[2]) : 1000;
    rng_state = seed * 0x9E3779B97F4A7C15ull + 1;
    refused_tables();
    for (int c = 0; c < cases; c++) {
        const uint32_t nb = (uint32_t)below(12); // 0 to 11 blocks, many of 1 byte
        std::vector<uint32_t> sizes(nb);
        uint64_t total = 0;
        for (uint32_t &s : sizes) total += s = below(3) ? 1 + (uint32_t)below(40) : 1;
        // the delimiters: none, all, or some -- and then often at a block's last byte and at the next one's first
        std::vector<uint8_t> isd(total, 0);
        const uint32_t mode = (uint32_t)below(8);
        for (uint64_t i = 0; i < total; i++) isd[i] = mode == 0 ? 0 : mode == 1 ? 1 : below(mode) == 0;
        if (mode >= 2) {
            uint64_t off = 0;
            for (uint32_t s : sizes) {
                off += s;
                if (off < total && below(2)) isd[off - 1] = 1;
                if (off < total && below(3) == 0) isd[off] = 1;
            }
        }
        uint64_t D = 0;
        for (uint8_t v : isd) D += v;
        // 0 to 40 ascending ranges with empty and adjacent ones, ones behind D, and lengths up to 2^64 - 1
        std::vector<bzh_range> ranges((size_t)below(41));
        uint64_t at = 0;
        for (bzh_range &r : ranges) {
            at += below(3) ? 0 : below(D / 4 + 2);
            r.off = at;
            r.len = below(9) == 0 ? ~0ull - below(3) : below(5) == 0 ? 0 : below(D / 3 + 3);
            if (below(30) == 0) r.off = std::max(at, D + below(4));
            at = sat_add(r.off, r.len) < D + 5 ? sat_add(r.off, r.len) : D + 5;
        }
        const bool shuffle = below(6) == 0 && ranges.size() > 1; // every list that does not ascend is refused
        if (shuffle) std::swap(ranges[below(ranges.size())], ranges[below(ranges.size())]);
        records_case(sizes, isd, ranges, 1 + (uint32_t)below(5), 1 + (uint32_t)below(4), !shuffle);
    }
    printf("records_host: %d cases held\n", cases);
    return 0;
}
