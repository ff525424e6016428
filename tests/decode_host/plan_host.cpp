// plan_host.cpp -- the decoder's host arithmetic (banzai_amd/csrc/decode_plan.h: tile prefix sums, the window of a range inside
// an index entry, the segment list of a batch) against brute force, built with g++ -fsanitize=address,undefined.  decode.hip
// calls the same text; there a wrong offset is a store outside a buffer on the device, here it is a failed comparison or a
// sanitizer report.  Every array is a heap allocation of exactly the size the function may touch.
//
//   plan_host <seed> <cases>     exit status 0: all three held for <cases> seeded cases each (and the fixed ones)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

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
            fprintf(stderr, "plan_host: %s: ", #cond);        \
            fprintf(stderr, __VA_ARGS__);                     \
            fprintf(stderr, "\n");                            \
            exit(1);                                          \
        }                                                     \
    } while (0)

// ---- tile prefix sums against a running loop ----------------------------------------------------------------------
static void sums_case(uint32_t nblock, uint32_t tile, uint32_t spare)
{
    const uint32_t tn = (uint32_t)(((uint64_t)nblock + tile - 1) / tile);
    std::vector<uint32_t> tout(tn); // exactly the tiles of the block: one read further is a report
    for (uint32_t &v : tout) v = (uint32_t)below(below(4) ? 300 : 1100000);
    const uint32_t mark = 0xDEADBEEFu;
    std::vector<uint32_t> toff(tn + spare, mark);
    const uint64_t got = bzp_tile_sums(tout.data(), toff.data(), nblock, tile);
    uint64_t run = 0;
    for (uint32_t t = 0; t < tn; t++) {
        CHECK(toff[t] == (uint32_t)run, "nblock %u tile %u: toff[%u] = %u, the running sum %llu", nblock, tile, t, toff[t], (unsigned long long)run);
        run += tout[t];
    }
    CHECK(got == run, "nblock %u tile %u: size %llu, the running sum %llu", nblock, tile, (unsigned long long)got, (unsigned long long)run);
    for (uint32_t t = tn; t < tn + spare; t++) CHECK(toff[t] == mark, "nblock %u tile %u: tile %u behind the block was written", nblock, tile, t);
}

static void check_sums(size_t cases)
{
    const uint32_t tiles[] = {1, 3, 16, 4096};
    for (uint32_t tile : tiles)
        for (uint32_t nblock : {0u, 1u, tile - 1, tile, tile + 1, 7 * tile, 7 * tile + 1, 8 * tile - 1}) sums_case(nblock, tile, 2);
    sums_case(900000, 4096, 0); // the largest block: 220 tiles, the last one short
    for (size_t c = 0; c < cases; c++) {
        const uint32_t tile = tiles[below(4)];
        sums_case((uint32_t)below((uint64_t)tile * 40 + 2), tile, (uint32_t)below(3));
    }
}

// ---- the window of a range inside an entry, byte by byte ----------------------------------------------------------
// entries of `sizes` back to back from 0, the range [off, off + len) clipped to their total as decode_range_run clips it
static void window_case(const std::vector<uint32_t> &sizes, uint64_t off, uint64_t len)
{
    uint64_t total = 0;
    for (uint32_t s : sizes) total += s;
    const uint64_t clipped = off < total ? (len < total - off ? len : total - off) : 0, end = off + clipped;
    std::vector<uint32_t> hits(clipped, 0); // the output buffer: how often each of its bytes is written
    uint64_t out_off = 0, wanted = 0;
    for (size_t k = 0; k < sizes.size(); k++) {
        const uint32_t out_len = sizes[k];
        uint32_t lo = 77, hi = 77;
        const bool whole = bzp_window(out_off, out_len, off, end, &lo, &hi);
        uint32_t count = 0, first = 0;
        for (uint32_t j = 0; j < out_len; j++)
            if (out_off + j >= off && out_off + j < end) {
                if (!count) first = j;
                count++;
            }
        CHECK(lo <= hi && hi <= out_len, "entry %zu [%llu, +%u) range [%llu, %llu): window [%u, %u)", k, (unsigned long long)out_off, out_len,
              (unsigned long long)off, (unsigned long long)end, lo, hi);
        CHECK(hi - lo == count && (!count || lo == first), "entry %zu [%llu, +%u) range [%llu, %llu): window [%u, %u), %u bytes from %u belong", k,
              (unsigned long long)out_off, out_len, (unsigned long long)off, (unsigned long long)end, lo, hi, count, first);
        CHECK(whole == (count == out_len), "entry %zu of %u bytes, %u wanted: whole = %d", k, out_len, count, (int)whole);
        const int64_t base = (int64_t)out_off - (int64_t)off; // where decode_range_run puts the entry's first byte
        for (uint32_t j = lo; j < hi; j++) {
            const int64_t at = base + j;
            CHECK(at >= 0 && (uint64_t)at < clipped, "entry %zu: byte %u lands at %lld of a buffer of %llu", k, j, (long long)at, (unsigned long long)clipped);
            hits[(size_t)at]++;
        }
        wanted += count;
        out_off += out_len;
    }
    CHECK(wanted == clipped, "%llu bytes wanted, the range holds %llu", (unsigned long long)wanted, (unsigned long long)clipped);
    for (uint64_t i = 0; i < clipped; i++) CHECK(hits[i] == 1, "output byte %llu written %u times", (unsigned long long)i, hits[i]);
}

static void check_windows(size_t cases)
{
    for (size_t c = 0; c < cases; c++) {
        std::vector<uint32_t> sizes(1 + below(9));
        for (uint32_t &s : sizes) s = below(4) ? (uint32_t)below(40) : 0; // entries of size 0 among them
        uint64_t total = 0;
        for (uint32_t s : sizes) total += s;
        const size_t edge = below(sizes.size() + 1); // a block edge: the start of entry `edge`, or the total
        uint64_t edge_at = 0;
        for (size_t k = 0; k < edge; k++) edge_at += sizes[k];
        window_case(sizes, below(total + 3), below(total + 5));                   // anywhere; `off` beyond the total among them
        const uint64_t o = below(edge_at + 1);
        window_case(sizes, o, edge_at - o);                                       // ends exactly on a block edge
        window_case(sizes, edge_at, below(total + 5));                            // starts exactly on one
        window_case(sizes, total + below(3), 1 + below(9));                       // `off` at and beyond the total
        window_case(sizes, 0, total);                                             // everything: every entry whole
        window_case(sizes, below(total + 1), ~0ull - total - 8);                  // a length far beyond the end
    }
    // the function alone, away from a running index: a range wholly in front of and wholly behind the entry, and offsets near 2^64
    uint32_t lo, hi;
    CHECK(!bzp_window(100, 10, 0, 100, &lo, &hi) && lo == hi, "a range that ends where the entry starts: [%u, %u)", lo, hi);
    CHECK(!bzp_window(100, 10, 110, 500, &lo, &hi) && lo == hi, "a range that starts where the entry ends: [%u, %u)", lo, hi);
    CHECK(!bzp_window(100, 10, 500, 600, &lo, &hi) && lo == hi, "a range behind the entry: [%u, %u)", lo, hi);
    CHECK(bzp_window(~0ull - 20, 10, 5, ~0ull, &lo, &hi) && lo == 0 && hi == 10, "an entry near 2^64: [%u, %u)", lo, hi);
    CHECK(!bzp_window(~0ull - 20, 10, ~0ull - 17, ~0ull - 12, &lo, &hi) && lo == 3 && hi == 8, "a window near 2^64: [%u, %u)", lo, hi);
}

// ---- the segment list of a batch ----------------------------------------------------------------------------------
// per[k]: the points of block k of the batch (entry e0 + k); before / behind: points of entries outside the batch
static void segments_case(size_t e0, const std::vector<uint32_t> &per, uint32_t before, uint32_t behind)
{
    const uint32_t B = (uint32_t)per.size();
    std::vector<bzh_index_entry> idx(e0 + B); // exactly the entries up to the batch's last
    for (bzh_index_entry &e : idx) e.level = 1 + (uint32_t)below(9);
    std::vector<bzh_sync_point> pts;
    bzh_sync_point p = {};
    for (uint32_t i = 0; i < (e0 ? before : 0); i++) {
        p.entry = (uint32_t)(e0 - 1);
        pts.push_back(p);
    }
    const size_t p0 = pts.size();
    for (uint32_t k = 0; k < B; k++)
        for (uint32_t i = 0; i < per[k]; i++) {
            p.entry = (uint32_t)(e0 + k);
            pts.push_back(p);
        }
    const size_t p1 = pts.size();
    for (uint32_t i = 0; i < behind; i++) {
        p.entry = (uint32_t)(e0 + B);
        pts.push_back(p);
    }
    std::vector<SegDesc> segs(3, SegDesc{9, 9, 9, 9}); // (what an earlier batch left)
    std::vector<uint32_t> seg0(1, 5);
    std::vector<size_t> pmap(2, 7);
    std::vector<uint32_t> ent(B); // e0 .. e0 + B - 1
    for (uint32_t k = 0; k < B; k++) ent[k] = (uint32_t)(e0 + k);
    bzp_segments(idx.data(), ent.data(), B, pts.data(), pts.size(), segs, seg0, pmap);
    CHECK(seg0.size() == (size_t)B + 1 && seg0[0] == 0 && seg0[B] == segs.size(), "seg0 of %zu for %u blocks, ends at %u of %zu", seg0.size(), B,
          seg0.empty() ? 0 : seg0.back(), segs.size());
    CHECK(segs.size() == B + (p1 - p0), "%zu segments for %u blocks and %zu points", segs.size(), B, p1 - p0);
    CHECK(pmap.size() == p1 - p0, "%zu points gathered of %zu", pmap.size(), p1 - p0);
    for (size_t j = 0; j < pmap.size(); j++) CHECK(pmap[j] == p0 + j, "gathered point %zu is point %zu, not %zu", j, pmap[j], p0 + j);
    int32_t next_point = 0; // points are used once each, in order
    for (uint32_t k = 0; k < B; k++) {
        CHECK(seg0[k + 1] - seg0[k] == per[k] + 1, "block %u with %u points has %u segments", k, per[k], seg0[k + 1] - seg0[k]);
        int32_t from = -1; // every block starts at its header's state
        for (uint32_t g = seg0[k]; g < seg0[k + 1]; g++) {
            const SegDesc &d = segs[g];
            CHECK(d.slot == k && d.block_max == 100000u * idx[e0 + k].level, "segment %u: slot %u, room %u in block %u of level %u", g, d.slot,
                  d.block_max, k, idx[e0 + k].level);
            CHECK(d.from == from, "segment %u of block %u starts at point %d, the one in front of it ends at %d", g, k, d.from, from);
            if (g + 1 < seg0[k + 1]) {
                CHECK(d.to == next_point && (size_t)d.to < pmap.size() && pts[pmap[(size_t)d.to]].entry == e0 + k, "segment %u of block %u ends at point %d", g, k, d.to);
                next_point++;
            } else {
                CHECK(d.to == -1, "the last segment of block %u ends at point %d", k, d.to);
            }
            from = d.to;
        }
    }
    CHECK((size_t)next_point == p1 - p0, "%d of %zu points used", next_point, p1 - p0);
}

static void check_segments(size_t cases)
{
    for (size_t c = 0; c < cases; c++) {
        const uint32_t B = 1 + (uint32_t)below(8);
        std::vector<uint32_t> per(B, 0);
        const uint64_t shape = below(4);
        if (shape == 0)
            per[below(B)] = 1 + (uint32_t)below(12); // all points in one block
        else if (shape < 3)
            for (uint32_t &v : per) v = below(3) ? (uint32_t)below(5) : 0; // blocks with no point among them
        // (shape 3: no point at all)
        segments_case(below(4) ? below(50) : 0, per, (uint32_t)below(4), (uint32_t)below(4));
    }
}

int main(int argc, char **argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: plan_host <seed> <cases>\n");
        return 2;
    }
    rng_state = strtoull(argv[1], nullptr, 10) * 0x9E3779B97F4A7C15ull + 1;
    const size_t cases = (size_t)strtoull(argv[2], nullptr, 10);
    check_sums(cases);
    check_windows(cases);
    check_segments(cases);
    printf("plan_host: %zu cases each of tile sums, windows and segments held\n", cases);
    return 0;
}
