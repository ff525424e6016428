// count_host.cpp -- unrle_count and unrle_select (banzai_amd/csrc/decode.hip) thread by thread in the kernels' layout -- tiles of
// 4096 bytes behind the inverse BWT, 16 a thread, each thread entered in the state the scan hands it --, from the text
// decode_core.h shares with the kernels (bzd_ur_count, bzd_ur_select), against the serial expansion.  Built with
// g++ -fsanitize=address,undefined; the arrays are allocated at their exact sizes and never left.
//
//   count_host <seed> <blocks>     exit status 0: everything held for <blocks> seeded blocks (and the fixed ones)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../banzai_amd/csrc/decode_core.h"
#include "unrle_layout.h"

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
            fprintf(stderr, "count_host: %s: ", #cond);  \
            fprintf(stderr, __VA_ARGS__);                \
            fprintf(stderr, "\n");                       \
            exit(1);                                     \
        }                                                \
    } while (0)

constexpr uint32_t NONE = 0xFFFFFFFFu;

// The block as the kernels see it; returns the delimiters the model counted, and checks every tile, every k and the last-byte flag.
static uint64_t block_case(const std::vector<uint8_t> &x, uint32_t delim, const char *name)
{
    const uint32_t n = (uint32_t)x.size();
    CHECK(n >= 1, "%s: an empty block", name);
    const Serial truth = expand(x.data(), n);
    const std::vector<uint8_t> &out = truth.out;
    const std::vector<uint32_t> &begin = truth.begin;
    CHECK(truth.end != 4, "%s: the case ends in four equal bytes without a count", name);
    std::vector<uint32_t> dpos; // the positions of the delimiters
    for (uint32_t p = 0; p < out.size(); p++)
        if (out[p] == delim) dpos.push_back(p);

    std::vector<Tile> tiles;
    uint32_t bsize;
    CHECK(lay_out(x.data(), n, tiles, &bsize) == truth.end && bsize == out.size(), "%s: the layout's end state or size", name);
    const uint32_t tn = (uint32_t)tiles.size();
    uint64_t counted = 0;
    size_t dnext = 0; // delimiters of the tiles before this one
    uint32_t last_flag = NONE;
    for (uint32_t t = 0; t < tn; t++) {
        const std::vector<Thread> &th = tiles[t].th; // what ur_load and the scan hand the threads
        CHECK(th.size() == THREADS, "%s: tile %u has %zu threads", name, t, th.size());
        for (uint32_t j = 0; j < THREADS; j++)
            if (th[j].cnt) CHECK(th[j].state == truth.state[t * TILE + j * ITEMS], "%s: tile %u thread %u is entered in state %u", name, t, j, th[j].state);
        // unrle_count: a count a thread, summed; the thread that holds the block's last byte writes the flag
        std::vector<uint32_t> d(THREADS), o(THREADS);
        uint32_t tcount = 0, tout = 0;
        for (uint32_t j = 0; j < THREADS; j++) {
            uint32_t last = 256;
            d[j] = bzd_ur_count(th[j].w, th[j].cnt, th[j].prev, th[j].state, delim, &o[j], &last);
            const uint32_t i0 = t * TILE + j * ITEMS;
            if (th[j].cnt && i0 + th[j].cnt == n) {
                CHECK(last_flag == NONE, "%s: two threads hold the last byte", name);
                last_flag = last == delim;
            }
            if (th[j].cnt) CHECK(o[j] == begin[i0 + th[j].cnt] - begin[i0], "%s: tile %u thread %u expands to %u bytes", name, t, j, o[j]);
            tcount += d[j];
            tout += o[j];
        }
        const uint32_t toff = begin[t * TILE];
        CHECK(tiles[t].toff == toff && tiles[t].total == tout, "%s: tile %u is laid out at %u with %u bytes", name, t, tiles[t].toff, tiles[t].total);
        uint32_t want = 0;
        for (uint32_t p = toff; p < toff + tout; p++) want += out[p] == delim;
        CHECK(tcount == want, "%s: tile %u counts %u delimiters, the expansion holds %u", name, t, tcount, want);
        // unrle_select: every k of the tile, and the two just outside
        for (uint32_t k = 0; k <= tcount + 1; k++) {
            uint32_t found = NONE, d0 = 0, o0 = 0, hits = 0;
            for (uint32_t j = 0; j < THREADS; j++) {
                if (k > d0 && k - d0 <= d[j]) {
                    const uint32_t at = bzd_ur_select(th[j].w, th[j].cnt, th[j].prev, th[j].state, delim, k - d0);
                    CHECK(at != NONE && at < o[j], "%s: tile %u thread %u does not find its delimiter %u", name, t, j, k - d0);
                    found = toff + o0 + at;
                    hits++;
                }
                d0 += d[j];
                o0 += o[j];
            }
            if (k == 0 || k > tcount) {
                CHECK(hits == 0 && found == NONE, "%s: tile %u answers query %u of %u", name, t, k, tcount);
                continue;
            }
            CHECK(hits == 1, "%s: tile %u, k %u: %u threads answer", name, t, k, hits);
            CHECK(found == dpos[dnext + k - 1], "%s: tile %u, k %u: position %u, the expansion says %u", name, t, k, found, dpos[dnext + k - 1]);
        }
        // a thread asked for more than it holds, or for nothing, says so
        for (uint32_t j = 0; j < THREADS; j += 37) {
            CHECK(bzd_ur_select(th[j].w, th[j].cnt, th[j].prev, th[j].state, delim, d[j] + 1) == NONE, "%s: k beyond a thread's count", name);
            CHECK(bzd_ur_select(th[j].w, th[j].cnt, th[j].prev, th[j].state, delim, 0) == NONE, "%s: k 0", name);
        }
        dnext += tcount;
        counted += tcount;
    }
    CHECK(counted == dpos.size(), "%s: %llu delimiters counted, %zu in the expansion", name, (unsigned long long)counted, dpos.size());
    CHECK(last_flag == (uint32_t)(out.back() == delim), "%s: the last-byte flag is %u", name, last_flag);
    return counted;
}

static std::vector<uint8_t> bytes(const std::string &s) { return std::vector<uint8_t>(s.begin(), s.end()); }

static void fixed_cases()
{
    // the count byte equals the delimiter: a count byte is never a literal
    CHECK(block_case(bytes("aaaa\x0a"), 10, "aaaa+10") == 0, "fourteen a hold no newline");
    CHECK(block_case(bytes("\n\n\n\n\x03"), 10, "nnnn+3") == 7, "seven newlines");
    CHECK(block_case(bytes("\n\n\n\n\x0a"), 10, "nnnn+10") == 14, "fourteen newlines");
    // count bytes 0 and 255
    CHECK(block_case(bytes(std::string("\n\n\n\n") + std::string(1, '\0')), 10, "nnnn+0") == 4, "a count of 0");
    CHECK(block_case(bytes(std::string("\n\n\n\n") + std::string(1, '\0') + "b"), 10, "nnnn+0+b") == 4, "a count of 0, then a literal");
    CHECK(block_case(bytes("\n\n\n\n\xff"), 10, "nnnn+255") == 259, "every k of a 259-byte run");
    CHECK(block_case(bytes("x\n\n\n\n\xffy\n"), 10, "x+run+y") == 260, "a run inside a block");
    // a block of one byte
    CHECK(block_case(bytes("\n"), 10, "one newline") == 1, "one byte");
    CHECK(block_case(bytes("a"), 10, "one a") == 0, "one byte");
    // the count byte is the first byte of the next thread, and of the next tile (entry state 4)
    for (uint32_t edge : {ITEMS, 5 * ITEMS, TILE, 2 * TILE}) {
        std::vector<uint8_t> x;
        for (uint32_t i = 0; i + 4 < edge; i++) x.push_back((uint8_t)("ab\ncd"[i % 5]));
        for (int i = 0; i < 4; i++) x.push_back(10);
        x.push_back(200);
        x.push_back('z');
        x.push_back(10);
        block_case(x, 10, "the count byte opens a thread or a tile");
    }
    // exactly one tile, and one byte more
    for (uint32_t n : {TILE, TILE + 1}) {
        std::vector<uint8_t> x(n);
        for (uint32_t i = 0; i < n; i++) x[i] = (uint8_t)(i % 7 == 3 ? 10 : 'a' + i % 5);
        block_case(x, 10, "one tile, and one byte more");
    }
    // the delimiter 0 and the delimiter 255
    block_case(bytes(std::string(4, '\0') + "\x05" + "q" + std::string(1, '\0')), 0, "delimiter 0");
    block_case(bytes("\xff\xff\xff\xff\x02\xff"), 255, "delimiter 255");
}

int main(int argc, char **argv)
{
    const uint64_t seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    const int blocks = argc > 2 ? atoi(argv[2]) : 100;
    rng_state = seed * 0x9E3779B97F4A7C15ull + 1;
    fixed_cases();
    for (int c = 0; c < blocks; c++) {
        const uint32_t n = 1 + (uint32_t)below(12286), delim = below(4) ? 10 : (uint32_t)below(256);
        const bool runny = c & 1;
        const uint8_t alpha[6] = {(uint8_t)delim, 'a', 'b', 3, 0, 255};
        std::vector<uint8_t> x;
        while (x.size() < n) {
            if (below(runny ? 3 : 40) == 0 && x.size() + 5 <= n) { // four equal bytes and their count, which may equal the delimiter
                const uint8_t v = alpha[below(below(2) ? 1 : 6)];
                x.insert(x.end(), 4, v);
                x.push_back(below(3) ? (uint8_t)below(256) : (uint8_t)delim);
            } else {
                x.push_back(alpha[below(6)]);
            }
        }
        // (whatever the bytes are they are a block, unless it ends in four equal bytes without a count: then a count is the last)
        uint32_t s = 0, prev = 256;
        for (uint8_t v : x) {
            s = bzd_rl_step(s, v == prev);
            prev = v;
        }
        if (s == 4) x.push_back((uint8_t)below(256));
        block_case(x, delim, "seeded");
    }
    printf("count_host: %d seeded blocks held\n", blocks);
    return 0;
}
