// gather_host.cpp -- the per-word rule of bzh_recover_stream's gather (banzai_amd/csrc/recover_gather.h: descriptor search,
// two-word funnel, tail mask) against a bit-by-bit copy, built with g++ -fsanitize=address,undefined.  The kernel (recover.hip)
// runs the same text, a thread a destination word, the search once per 64 words: so does this.  The source and the output are
// heap arrays of exactly their size, so a read or a store one byte outside either is a report; the words the rule does not own
// are guard words and must stay as they were.
//
//   gather_host <seed> <lists>     exit status 0: every single block and every seeded list held
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../banzai_amd/csrc/decode_recover_plan.h" // bzr_report_check
#include "../../banzai_amd/csrc/recover_gather.h"

static uint64_t rng_state;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}
static uint64_t below(uint64_t n) { return n ? rnd() % n : 0; }

#define CHECK(cond, ...)                                     \
    do {                                                     \
        if (!(cond)) {                                       \
            fprintf(stderr, "gather_host: %s: ", #cond);     \
            fprintf(stderr, __VA_ARGS__);                    \
            fprintf(stderr, "\n");                           \
            exit(1);                                         \
        }                                                    \
    } while (0)

static int get_bit(const uint8_t *p, uint64_t bit) { return (p[bit >> 3] >> (7 - (bit & 7u))) & 1; }
static void set_bit(uint8_t *p, uint64_t bit, int v)
{
    if (v) p[bit >> 3] |= (uint8_t)(0x80u >> (bit & 7u));
}

// The blocks (source bit, bits) laid end to end from destination bit `dst0` on, by the rule as the kernel applies it: words
// [dst0 / 32 .., the word of the last bit], a search per group of 64 words.  Words outside: guards.
static void run_list(const std::vector<uint8_t> &srcv, const std::vector<BzrDesc> &d, uint64_t dst0, bool per_word)
{
    uint64_t body = 0;
    for (const BzrDesc &x : d) body += x.nbits;
    const uint64_t end = dst0 + body, w0 = dst0 / 32, wend = (end + 31) / 32;
    const size_t guard = 4; // words in front and behind
    uint32_t *out = (uint32_t *)malloc((size_t)(wend - w0 + 2 * guard) * 4);
    const uint32_t G = 0xA5C3F00Du;
    for (size_t i = 0; i < (size_t)(wend - w0) + 2 * guard; i++) out[i] = G;
    uint8_t *src = (uint8_t *)malloc(srcv.size() ? srcv.size() : 1); // exactly the input: one byte further is a report
    if (!srcv.empty()) memcpy(src, srcv.data(), srcv.size());
    uint32_t *base = out + guard - w0; // base[word]
    for (uint64_t g = w0 / 64 * 64; g < wend; g += 64) { // (the kernel's wavefronts: 64 words from a multiple of 64 on)
        const uint32_t k0 = bzr_find(d.data(), (uint32_t)d.size(), g * 32);
        for (uint64_t word = g < w0 ? w0 : g; word < wend && word < g + 64; word++) {
            const uint32_t k = per_word ? bzr_find(d.data(), (uint32_t)d.size(), word * 32) : k0;
            base[word] = __builtin_bswap32(bzr_gather_word(d.data(), (uint32_t)d.size(), k, word, src, srcv.size()));
        }
    }
    // the bit-by-bit copy
    std::vector<uint8_t> want((size_t)(wend - w0) * 4, 0);
    uint64_t at = dst0 - w0 * 32;
    for (const BzrDesc &x : d)
        for (uint64_t b = 0; b < x.nbits; b++) set_bit(want.data(), at++, get_bit(src, x.src_bit + b));
    CHECK(!memcmp(want.data(), base + w0, want.size()), "%zu blocks from destination bit %llu: the words differ from the bit-by-bit copy", d.size(),
          (unsigned long long)dst0);
    for (size_t i = 0; i < guard; i++) CHECK(out[i] == G && out[guard + (wend - w0) + i] == G, "a guard word was written");
    free(src);
    free(out);
}

int main(int argc, char **argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: gather_host <seed> <lists>\n");
        return 2;
    }
    rng_state = strtoull(argv[1], nullptr, 10) * 0x9E3779B97F4A7C15ull + 1;
    const size_t lists = strtoull(argv[2], nullptr, 10);
    // single blocks: every source residue, every destination residue, 1..130 bits; the source ends with the block's last bit
    for (uint32_t sr = 0; sr < 32; sr++)
        for (uint32_t dr = 0; dr < 32; dr++)
            for (uint32_t len = 1; len <= 130; len++) {
                std::vector<uint8_t> src((sr + len + 7) / 8);
                for (uint8_t &b : src) b = (uint8_t)rnd();
                run_list(src, {BzrDesc{sr, 32 + dr, len}}, 32 + dr, (sr + dr + len) & 1);
            }
    // lists of 1..40 blocks of 81 bits and more, in a source with gaps between them; the first may start at bit 0, the last end
    // in the last bits of the buffer
    for (size_t c = 0; c < lists; c++) {
        const uint32_t K = 1 + (uint32_t)below(40);
        std::vector<BzrDesc> d;
        std::vector<bzh_recover_entry> ent;
        uint64_t sbit = below(3) ? below(70) : 0, dbit = 32;
        for (uint32_t k = 0; k < K; k++) {
            const uint64_t len = 81 + (below(4) ? below(200) : below(5000));
            d.push_back(BzrDesc{sbit, dbit, len});
            bzh_recover_entry e{};
            e.bit_pos = sbit, e.end_bit = sbit + len;
            ent.push_back(e);
            if (below(3) == 0) { // a lost entry between them
                bzh_recover_entry l{};
                l.bit_pos = sbit + 49, l.kind = BZH_LOST_FORMAT;
                ent.push_back(l);
            }
            dbit += len;
            sbit += len + (below(2) ? below(300) : 0);
        }
        const uint64_t last_end = d.back().src_bit + d.back().nbits;
        const size_t n = (size_t)((last_end + 7) / 8) + (below(2) ? 0 : (size_t)below(9));
        std::vector<uint8_t> src(n);
        for (uint8_t &b : src) b = (uint8_t)rnd();
        size_t bad = 0, kept = 0;
        uint64_t body = 0;
        CHECK(bzr_report_check(ent.data(), ent.size(), n, &bad, &body, &kept) == nullptr && kept == K && body == dbit - 32, "a well-formed report is refused at %zu", bad);
        run_list(src, d, 32, c & 1);
        // what the check refuses: each of the four, and it names the entry
        std::vector<bzh_recover_entry> e2 = ent;
        size_t ki = 0;
        for (size_t i = 0; i < e2.size(); i++)
            if (e2[i].kind == 0) ki = i;
        e2[ki].end_bit = 8 * (uint64_t)n + 1;
        CHECK(bzr_report_check(e2.data(), e2.size(), n, &bad, &body, &kept) && bad == ki, "an end behind the input is accepted");
        e2 = ent;
        e2[ki].end_bit = e2[ki].bit_pos + 80;
        CHECK(bzr_report_check(e2.data(), e2.size(), n, &bad, &body, &kept) && bad == ki, "a block of 80 bits is accepted");
        e2 = ent;
        e2[ki].kind = BZH_LOST_TRUNC;
        CHECK(bzr_report_check(e2.data(), e2.size(), n, &bad, &body, &kept) && bad == ki, "a lost entry with an end is accepted");
        if (K >= 2) {
            e2 = ent;
            size_t first_kept = 0;
            while (e2[first_kept].kind != 0) first_kept++;
            e2[ki].bit_pos = e2[first_kept].bit_pos; // overlaps what lies before it
            CHECK(bzr_report_check(e2.data(), e2.size(), n, &bad, &body, &kept) && bad > first_kept, "overlapping entries are accepted");
        }
    }
    // descriptors the check would never pass: whatever they hold, no read leaves the source (zeros come back instead)
    {
        std::vector<uint8_t> src(10, 0xFF);
        run_list(src, {BzrDesc{0, 32, 80}}, 32, false); // exactly the buffer
        uint8_t *p = (uint8_t *)malloc(10);
        memset(p, 0xFF, 10);
        const BzrDesc wild[2] = {{72, 32, 40}, {1ull << 40, 72, 64}};
        CHECK(bzr_gather_word(wild, 2, 0, 1, p, 10) == 0xFF000000u, "bits behind the source are not zero");
        CHECK(bzr_gather_word(wild, 2, 0, 2, p, 10) == 0u && bzr_gather_word(wild, 2, 0, 3, p, 10) == 0u, "bits behind the source are not zero");
        free(p);
    }
    printf("gather_host: %zu lists held\n", lists);
    return 0;
}
