// pieces_host.cpp -- what unrle_walk_pieces (banzai_amd/csrc/decode.hip) does with the tables bzp_pieces builds, as a CPU
// program built with -fsanitize=address,undefined.  The kernel's per-thread text is decode_core.h's (bzd_ur_emit, bzd_piece_cut)
// and the tables are decode_plan.h's; the threads are laid out as the kernel lays them out (unrle_layout.h), with a stage of
// 8,192 bytes, and run one after the other:
// a tile that fits the stage is expanded into it once and copied to every piece that meets it, a larger one is emitted piece
// by piece.  The stage and the output are heap buffers of exactly their size: a store outside either is a sanitizer report.
//
//   pieces_host <seed> <cases>     exit status 0: every piece of every case held the bytes of the block's full expansion
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/bzhip.h"
#include "../../banzai_amd/csrc/decode_plan.h"
#include "unrle_layout.h"

constexpr uint32_t STAGE = 8192;

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
            fprintf(stderr, "pieces_host: %s: ", #cond);      \
            fprintf(stderr, __VA_ARGS__);                     \
            fprintf(stderr, "\n");                            \
            exit(1);                                          \
        }                                                     \
    } while (0)

// a block behind the inverse BWT: literals and runs, the counts behind four equal bytes small or (heavy) up to 255
static std::vector<uint8_t> make_block(uint32_t n, bool heavy)
{
    std::vector<uint8_t> x;
    while (x.size() < n) {
        const uint8_t c = (uint8_t)(97 + below(heavy ? 3 : 20));
        if (below(heavy ? 2 : 12) == 0) {
            x.insert(x.end(), 4, c);
            x.push_back((uint8_t)(heavy ? 200 + below(56) : below(9)));
        } else {
            x.push_back(c);
        }
    }
    x.resize(n);
    return x;
}

static void pieces_case(uint32_t n, bool heavy, uint32_t npieces)
{
    const std::vector<uint8_t> x = make_block(n, heavy);
    std::vector<Tile> tiles;
    uint32_t size;
    (void)lay_out(x.data(), n, tiles, &size);
    const std::vector<uint8_t> full = expand(x.data(), n).out;
    CHECK(full.size() == size, "the layout sums to %u bytes, the serial expansion has %zu", size, full.size());
    // pieces anywhere in the block, their destinations back to back: short ones, some in one tile, some over all of it
    std::vector<PieceRef> pc(npieces);
    uint64_t out_total = 0;
    const uint32_t spot = (uint32_t)below(size + 1);
    for (PieceRef &p : pc) {
        const uint32_t kind = (uint32_t)below(4);
        p.lo = kind == 0 ? (uint32_t)below(size + 1) : kind == 1 ? spot + (uint32_t)below(64) : kind == 2 ? 0 : (uint32_t)below(size + 1);
        p.lo = std::min(p.lo, size);
        p.hi = std::min<uint64_t>(size, (uint64_t)p.lo + (kind == 2 ? size : kind == 3 ? below(20000) : below(12)));
        p.base = out_total;
        out_total += p.hi - p.lo;
    }
    const uint32_t Tn = (uint32_t)tiles.size(), rows = 0, ntiles = Tn;
    std::vector<uint32_t> tout(Tn), toff(Tn), tile_first;
    for (uint32_t t = 0; t < Tn; t++) tout[t] = tiles[t].total, toff[t] = tiles[t].toff;
    const size_t pf[2] = {0, pc.size()};
    std::vector<PieceRef> refs;
    CHECK(bzp_pieces(&rows, &ntiles, 1, tout.data(), toff.data(), Tn, Tn, pf, pc.data(), tile_first, refs), "overflow");
    uint8_t *out = (uint8_t *)malloc(out_total ? out_total : 1), *stage = (uint8_t *)malloc(STAGE); // (exact sizes: ASan guards the ends)
    std::vector<uint32_t> hits(out_total, 0);
    for (uint32_t t = 0; t < Tn; t++) {
        const Tile &tl = tiles[t];
        const uint32_t f0 = tile_first[t], f1 = tile_first[t + 1];
        if (tl.total == 0 || f0 == f1) continue;
        const uint32_t lim = tl.total;
        const bool staged = tl.total <= STAGE;
        if (staged)
            for (const Thread &th : tl.th) bzd_ur_emit(th.w, th.cnt, th.prev, th.state, th.off, 0u, lim, [&](uint32_t q, uint8_t v) { stage[q] = v; });
        for (uint32_t f = f0; f < f1; f++) {
            uint32_t ca, cb;
            uint64_t dst;
            if (!bzd_piece_cut(tl.toff, lim, refs[f].lo, refs[f].hi, refs[f].base, out_total, &ca, &cb, &dst)) continue;
            uint8_t *g = out + dst;
            if (staged) {
                for (uint32_t q = ca; q < cb; q++) g[q - ca] = stage[q], hits[dst + q - ca]++;
            } else {
                for (const Thread &th : tl.th)
                    bzd_ur_emit(th.w, th.cnt, th.prev, th.state, th.off, ca, cb, [&](uint32_t q, uint8_t v) { g[q - ca] = v, hits[dst + q - ca]++; });
            }
        }
    }
    for (const PieceRef &p : pc) {
        for (uint32_t j = p.lo; j < p.hi; j++)
            CHECK(hits[p.base + j - p.lo] == 1 && out[p.base + j - p.lo] == full[j], "piece [%u, %u) of a block of %u bytes: byte %u written %u times",
                  p.lo, p.hi, size, j, hits[p.base + j - p.lo]);
    }
    // references that lie: outside the tile, outside the output -- nothing may be stored for them
    for (uint32_t t = 0; t < Tn && t < 3; t++) {
        uint32_t ca, cb;
        uint64_t dst;
        const Tile &tl = tiles[t];
        if (bzd_piece_cut(tl.toff, tl.total, 0, ~0u, out_total ? out_total - 1 : 0, out_total, &ca, &cb, &dst))
            CHECK(dst < out_total && cb - ca <= out_total - dst && cb <= tl.total, "a reference over everything stores %u bytes at %llu of %llu", cb - ca,
                  (unsigned long long)dst, (unsigned long long)out_total);
        CHECK(!bzd_piece_cut(tl.toff, tl.total, 0, ~0u, ~0ull - 2, out_total, &ca, &cb, &dst) || tl.total == 0 || out_total == 0 || dst < out_total,
              "a base at the end of the address space");
    }
    free(out);
    free(stage);
}

int main(int argc, char **argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: pieces_host <seed> <cases>\n");
        return 2;
    }
    rng_state = strtoull(argv[1], nullptr, 10) * 0x9E3779B97F4A7C15ull + 1;
    const size_t cases = (size_t)strtoull(argv[2], nullptr, 10);
    pieces_case(1, false, 3);
    pieces_case(TILE, false, 40);
    pieces_case(TILE + 1, true, 40);
    pieces_case(3 * TILE - 1, true, 1100); // more than a thousand pieces over tiles that do not fit the stage
    for (size_t c = 0; c < cases; c++) pieces_case(1 + (uint32_t)below(3 * TILE), below(2) != 0, (uint32_t)below(70));
    printf("pieces_host: the pieces of %zu seeded blocks held\n", cases);
    return 0;
}
