// ranges_host.cpp -- the host arithmetic of a call over many ranges (banzai_amd/csrc/decode_plan.h: bzp_spans, which is
// bzh_index_spans and the output layout of bzh_decode_ranges; bzp_block_pieces and bzp_pieces, which tell unrle_walk_pieces what to
// store where; bzp_segments over a list of entries) against brute force, built with g++ -fsanitize=address,undefined.  The brute
// force is per output byte: which ranges want it, and where it goes.  The decoded bytes of the synthetic index are their own
// positions, so a byte in the wrong place shows as a wrong value.
//
//   ranges_host <seed> <cases>     exit status 0: everything held for <cases> seeded cases (and the fixed ones)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <utility>
#include <vector>

#include "../../include/bzhip.h"
#include "../../banzai_amd/csrc/decode_plan.h"

static uint64_t rng_state;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}
static uint64_t below(uint64_t n) { return n ? rnd() % n : 0; }

#define CHECK(cond, ...)                                      \
    do {                                                      \
        if (!(cond)) {                                        \
            fprintf(stderr, "ranges_host: %s: ", #cond);      \
            fprintf(stderr, __VA_ARGS__);                     \
            fprintf(stderr, "\n");                            \
            exit(1);                                          \
        }                                                     \
    } while (0)

// An index of blocks of the given sizes (each at least 1), bit positions ascending with gaps, every third pair of neighbours
// sharing a byte.
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

static void ranges_case(const std::vector<uint32_t> &sizes, const std::vector<bzh_range> &ranges, uint32_t Bmax, uint32_t Tn)
{
    const std::vector<bzh_index_entry> idx = make_index(sizes);
    const size_t count = idx.size(), nr = ranges.size();
    uint64_t total = 0;
    for (uint32_t s : sizes) total += s;
    std::vector<uint32_t> entry_of(total);
    for (size_t k = 0; k < count; k++)
        for (uint32_t j = 0; j < sizes[k]; j++) entry_of[idx[k].out_off + j] = (uint32_t)k;

    // brute force, byte by byte: the expected output (the position every byte comes from), the touched entries, the pairs that meet
    std::vector<uint64_t> want, want_offs(nr), want_lens(nr);
    std::set<uint32_t> want_touched;
    std::set<std::pair<uint32_t, uint32_t>> want_pairs; // (entry, range)
    for (size_t r = 0; r < nr; r++) {
        want_offs[r] = want.size();
        for (uint64_t p = ranges[r].off, i = 0; p < total && i < ranges[r].len; p++, i++) {
            want.push_back(p);
            want_touched.insert(entry_of[p]);
            want_pairs.insert({entry_of[p], (uint32_t)r});
        }
        want_lens[r] = want.size() - want_offs[r];
    }

    // bzp_spans: exactly nr words each, exactly the entries
    std::vector<size_t> offs(nr), lens(nr);
    std::vector<uint32_t> touched;
    uint64_t blo = 77, bhi = 77;
    const uint64_t sum = bzp_spans(idx.data(), count, ranges.data(), nr, offs.data(), lens.data(), touched, &blo, &bhi);
    CHECK(sum == want.size(), "out_total %llu, byte by byte %zu", (unsigned long long)sum, want.size());
    for (size_t r = 0; r < nr; r++)
        CHECK(offs[r] == want_offs[r] && lens[r] == want_lens[r], "range %zu: at %zu holding %zu, byte by byte at %llu holding %llu", r, offs[r],
              lens[r], (unsigned long long)want_offs[r], (unsigned long long)want_lens[r]);
    CHECK(touched == std::vector<uint32_t>(want_touched.begin(), want_touched.end()), "the touched list differs (%zu entries, byte by byte %zu)",
          touched.size(), want_touched.size());
    if (touched.empty())
        CHECK(blo == 0 && bhi == 0, "nothing touched, bytes [%llu, %llu)", (unsigned long long)blo, (unsigned long long)bhi);
    else
        CHECK(blo == idx[touched.front()].bit_pos / 8 && bhi == (idx[touched.back()].end_bit + 7) / 8, "the hull [%llu, %llu)",
              (unsigned long long)blo, (unsigned long long)bhi);
    // with no room for offsets and lengths: the same sum and list
    std::vector<uint32_t> touched2;
    CHECK(bzp_spans(idx.data(), count, ranges.data(), nr, nullptr, nullptr, touched2, &blo, &bhi) == sum && touched2 == touched, "null arrays");

    // bzp_block_pieces: one piece per pair that meets, in the order of the ranges
    std::vector<size_t> pfirst;
    std::vector<PieceRef> pc;
    std::vector<uint32_t> prange;
    bzp_block_pieces(idx.data(), count, ranges.data(), nr, offs.data(), touched, pfirst, pc, prange);
    CHECK(pfirst.size() == touched.size() + 1 && pc.size() == want_pairs.size() && prange.size() == pc.size(), "%zu pieces, byte by byte %zu",
          pc.size(), want_pairs.size());
    for (size_t j = 0; j < touched.size(); j++)
        for (size_t q = pfirst[j]; q < pfirst[j + 1]; q++) {
            CHECK(want_pairs.count({touched[j], prange[q]}), "piece %zu: entry %u and range %u do not meet", q, touched[j], prange[q]);
            CHECK(q == pfirst[j] || prange[q - 1] < prange[q], "piece %zu: the ranges of entry %u do not ascend", q, touched[j]);
            CHECK(pc[q].lo < pc[q].hi && pc[q].hi <= sizes[touched[j]], "piece %zu: [%u, %u) of %u bytes", q, pc[q].lo, pc[q].hi, sizes[touched[j]]);
        }

    // bzp_pieces, batch by batch as the driver runs it, every touched block piece by piece: the stores it describes, carried out
    std::vector<uint64_t> out(want.size(), ~0ull);
    std::vector<uint32_t> hits(want.size(), 0);
    const uint32_t stride = Tn + (uint32_t)below(3);
    for (size_t t0 = 0; t0 < touched.size();) {
        const uint32_t K = (uint32_t)std::min<size_t>(Bmax, touched.size() - t0);
        std::vector<uint32_t> rows(K), ntiles(K), tout((size_t)K * stride, 0xDEADBEEFu), toff((size_t)K * stride, 0xDEADBEEFu);
        std::vector<size_t> pf(1, 0);
        std::vector<PieceRef> bpc;
        for (uint32_t k = 0; k < K; k++) {
            rows[k] = K - 1 - k; // (the rows need not be in the order of the blocks)
            ntiles[k] = 1 + (uint32_t)below(Tn);
            uint32_t *o = tout.data() + (size_t)rows[k] * stride, *f = toff.data() + (size_t)rows[k] * stride;
            make_tiles(sizes[touched[t0 + k]], ntiles[k], o);
            uint32_t run = 0;
            for (uint32_t t = 0; t < ntiles[k]; t++) f[t] = run, run += o[t];
            bpc.insert(bpc.end(), pc.begin() + pfirst[t0 + k], pc.begin() + pfirst[t0 + k + 1]);
            pf.push_back(bpc.size());
        }
        std::vector<uint32_t> tile_first;
        std::vector<PieceRef> refs;
        CHECK(bzp_pieces(rows.data(), ntiles.data(), K, tout.data(), toff.data(), stride, Tn, pf.data(), bpc.data(), tile_first, refs), "overflow");
        CHECK(tile_first.size() == (size_t)K * Tn + 1 && tile_first[0] == 0 && tile_first.back() == refs.size(), "the table's shape");
        for (uint32_t k = 0; k < K; k++)
            for (uint32_t t = 0; t < Tn; t++) {
                const size_t cell = (size_t)k * Tn + t;
                CHECK(tile_first[cell] <= tile_first[cell + 1], "tile_first descends at block %u tile %u", k, t);
                if (t >= ntiles[k]) {
                    CHECK(tile_first[cell] == tile_first[cell + 1], "a tile behind the block's last has references");
                    continue;
                }
                const uint32_t f = toff[(size_t)rows[k] * stride + t], o = tout[(size_t)rows[k] * stride + t];
                for (uint32_t q = tile_first[cell]; q < tile_first[cell + 1]; q++) {
                    const PieceRef &p = refs[q];
                    CHECK(p.lo < p.hi && p.lo >= f && p.hi <= f + o, "block %u tile %u at %u of %u bytes: reference [%u, %u)", k, t, f, o, p.lo, p.hi);
                    for (uint32_t j = p.lo; j < p.hi; j++) {
                        const uint64_t dst = p.base + (j - p.lo);
                        CHECK(dst < out.size(), "a store at %llu of %zu bytes", (unsigned long long)dst, out.size());
                        out[dst] = idx[touched[t0 + k]].out_off + j;
                        hits[dst]++;
                    }
                }
            }
        t0 += K;
    }
    for (size_t i = 0; i < want.size(); i++)
        CHECK(hits[i] == 1 && out[i] == want[i], "output byte %zu: written %u times, from %llu, wanted from %llu", i, hits[i],
              (unsigned long long)out[i], (unsigned long long)want[i]);
}

static std::vector<bzh_range> random_ranges(uint64_t total, size_t nr)
{
    std::vector<bzh_range> ranges(nr);
    for (bzh_range &r : ranges) {
        r.off = below(8) ? below(total + 1) : total + below(5);
        switch (below(8)) {
        case 0: r.len = 0; break;
        case 1: r.len = ~0ull - r.off; break; // ends at 2^64 - 1
        case 2: r.len = ~0ull; break;         // would end behind it
        case 3: r.len = total; break;
        default: r.len = below(below(2) ? 4 : total / 2 + 2); break;
        }
        if (below(6) == 0 && &r != &ranges[0]) r = (&r)[-1]; // a repeat
    }
    return ranges;
}

static void check_ranges(size_t cases)
{
    // fixed: no entries, no ranges, blocks of one byte, one block
    ranges_case({}, {}, 2, 3);
    ranges_case({}, {{0, 5}, {3, ~0ull}}, 2, 3);
    ranges_case({5, 7}, {}, 2, 3);
    ranges_case({1, 1, 1, 1, 1}, {{0, 5}, {4, 1}, {2, 0}, {1, 3}, {5, 1}, {0, ~0ull}}, 2, 1);
    ranges_case({40}, {{0, 40}, {39, 1}, {0, 1}, {13, ~0ull - 13}}, 1, 7);
    for (size_t c = 0; c < cases; c++) {
        std::vector<uint32_t> sizes(below(12));
        uint64_t total = 0;
        for (uint32_t &s : sizes) total += s = below(4) ? 1 + (uint32_t)below(60) : 1;
        ranges_case(sizes, random_ranges(total, below(65)), 1 + (uint32_t)below(5), 1 + (uint32_t)below(9));
    }
}

// ---- the segments of a batch given as a list of entries ---------------------------------------------------------------------
static void segments_case(uint32_t count, uint32_t maxpts, bool adjacent)
{
    std::vector<bzh_index_entry> idx(count);
    for (bzh_index_entry &e : idx) e.level = 1 + (uint32_t)below(9);
    std::vector<bzh_sync_point> pts;
    for (uint32_t e = 0; e < count; e++)
        for (uint32_t g = 0, n = (uint32_t)below(maxpts + 1); g < n; g++) {
            bzh_sync_point p{};
            p.entry = e;
            p.group = g + 1;
            pts.push_back(p);
        }
    std::vector<uint32_t> ent; // an ascending list of entries
    const uint32_t e0 = (uint32_t)below(count);
    for (uint32_t e = e0; e < count; e++)
        if (adjacent ? e < e0 + 4 : below(2) != 0) ent.push_back(e);
    std::vector<SegDesc> segs;
    std::vector<uint32_t> seg0;
    std::vector<size_t> pmap;
    bzp_segments(idx.data(), ent.data(), (uint32_t)ent.size(), pts.data(), pts.size(), segs, seg0, pmap);
    CHECK(seg0.size() == ent.size() + 1 && seg0.back() == segs.size(), "seg0's shape");
    size_t j = 0; // the gathered points met so far
    for (uint32_t k = 0; k < ent.size(); k++) {
        std::vector<size_t> own; // brute force: the points of the entry, in order
        for (size_t q = 0; q < pts.size(); q++)
            if (pts[q].entry == ent[k]) own.push_back(q);
        CHECK(seg0[k + 1] - seg0[k] == own.size() + 1, "entry %u: %u segments for %zu points", ent[k], seg0[k + 1] - seg0[k], own.size());
        int32_t prev = -1;
        for (uint32_t g = seg0[k]; g < seg0[k + 1]; g++) {
            const SegDesc &d = segs[g];
            const bool last = g + 1 == seg0[k + 1];
            CHECK(d.slot == k && d.block_max == 100000u * idx[ent[k]].level && d.from == prev, "segment %u of entry %u", g, ent[k]);
            CHECK(last ? d.to == -1 : d.to == (int32_t)j, "segment %u runs to %d", g, d.to);
            if (!last) {
                CHECK(j < pmap.size() && pmap[j] == own[g - seg0[k]], "gathered point %zu is not point %zu", j, own[g - seg0[k]]);
                prev = (int32_t)j++;
            }
        }
    }
    CHECK(j == pmap.size(), "%zu gathered points, %zu met", pmap.size(), j);
    if (adjacent && !ent.empty()) { // a single range's batch: its points are the run [p0, p1) of the array, every one of them used
        size_t p0 = 0, p1 = 0;
        while (p0 < pts.size() && pts[p0].entry < ent.front()) p0++;
        for (p1 = p0; p1 < pts.size() && pts[p1].entry <= ent.back(); p1++) {}
        CHECK(pmap.size() == p1 - p0 && segs.size() == ent.size() + (p1 - p0), "%zu points gathered and %zu segments for %zu blocks and %zu points",
              pmap.size(), segs.size(), ent.size(), p1 - p0);
        for (size_t q = 0; q < pmap.size(); q++) CHECK(pmap[q] == p0 + q, "an adjacent batch's points are not a run");
        // (so from / to, which the loop above has held to the gathered numbering, are the points' numbers counted from p0)
    }
}

static void check_segments(size_t cases)
{
    segments_case(1, 0, true);
    segments_case(1, 5, false);
    segments_case(9, 0, false);
    for (size_t c = 0; c < cases; c++) segments_case(1 + (uint32_t)below(12), (uint32_t)below(6), below(2) != 0);
}

int main(int argc, char **argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: ranges_host <seed> <cases>\n");
        return 2;
    }
    rng_state = strtoull(argv[1], nullptr, 10) * 0x9E3779B97F4A7C15ull + 1;
    const size_t cases = (size_t)strtoull(argv[2], nullptr, 10);
    check_ranges(cases);
    check_segments(cases);
    printf("ranges_host: bzp_spans, bzp_block_pieces, bzp_pieces and bzp_segments over a list held for %zu cases each\n", cases);
    return 0;
}
