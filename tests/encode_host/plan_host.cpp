// plan_host.cpp -- the encoder's host arithmetic (banzai_amd/csrc/encode_plan.h: the job split, a job's sums, the words zeroed
// before a pack, the inputs a batch of a many-streams call closes) against brute force, built with
// g++ -fsanitize=address,undefined.  api.hip's encode drivers call the same text; there a wrong word index is a bit ORed into a
// word that was never zeroed, here it is a failed comparison or a sanitizer report.  Every array is a heap allocation of exactly
// the size the function may touch.
//
//   plan_host <seed> <cases>     exit status 0: all four held for <cases> seeded cases each (and the fixed ones)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../banzai_amd/csrc/encode_plan.h"

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

// ---- the job split --------------------------------------------------------------------------------------------------
static void split_case(size_t b0, size_t nb, uint32_t lane_mb, size_t NL)
{
    // the rule, counted out: batches of lane_mb until nothing is left, a job for every lane where there are blocks enough,
    // then the smallest job size with which that many jobs hold all blocks
    size_t njobs = 0;
    for (size_t left = nb; left > 0; left -= (left < lane_mb ? left : lane_mb)) njobs++;
    if (njobs < NL && nb >= NL) njobs = NL;
    size_t per = 0;
    while (per * njobs < nb) per++;
    const size_t got = bze_per(nb, lane_mb, NL);
    CHECK(got == per, "nb %zu lane_mb %u NL %zu: per %zu, counted out %zu", nb, lane_mb, NL, got, per);
    std::vector<BzeSpan> jobs(2, BzeSpan{77, 77}); // (what an earlier call left)
    bze_split(b0, b0 + nb, got, jobs);
    size_t at = b0;
    for (const BzeSpan &j : jobs) {
        CHECK(j.k0 == at, "nb %zu lane_mb %u NL %zu: a job starts at %zu, the one in front of it ends at %zu", nb, lane_mb, NL, j.k0, at);
        CHECK(j.B >= 1 && j.B <= lane_mb, "nb %zu lane_mb %u NL %zu: a job of %u blocks", nb, lane_mb, NL, j.B);
        at += j.B;
    }
    CHECK(at == b0 + nb, "nb %zu lane_mb %u NL %zu: the jobs end at %zu, the range at %zu", nb, lane_mb, NL, at, b0 + nb);
    CHECK(jobs.size() <= njobs && (nb == 0) == jobs.empty(), "nb %zu lane_mb %u NL %zu: %zu jobs, at most %zu", nb, lane_mb, NL, jobs.size(), njobs);
    if (NL == 2 && nb >= 2) CHECK(jobs.size() >= 2, "nb %zu lane_mb %u: two lanes, %zu job", nb, lane_mb, jobs.size());
}

static void check_split(size_t cases)
{
    for (uint32_t lane_mb : {1u, 2u, 3u, 8u, 512u})
        for (size_t NL : {(size_t)1, (size_t)2})
            for (size_t nb : {(size_t)1, (size_t)2, (size_t)lane_mb, (size_t)lane_mb + 1, (size_t)2 * lane_mb, (size_t)2 * lane_mb + 1})
                for (size_t b0 : {(size_t)0, (size_t)5}) split_case(b0, nb, lane_mb, NL);
    for (size_t c = 0; c < cases; c++) {
        const uint32_t lane_mb = 1 + (uint32_t)below(below(3) ? 6 : 600);
        split_case(below(40), below((uint64_t)lane_mb * 4 + 3), lane_mb, 1 + below(2));
    }
}

// ---- a job's sums ---------------------------------------------------------------------------------------------------
struct Blk {
    uint64_t in_len;
    uint32_t rle_len;
};

static void check_sums(size_t cases)
{
    for (size_t c = 0; c < cases; c++) {
        const size_t k0 = below(6);
        const uint32_t B = (uint32_t)below(9);
        std::vector<Blk> blocks(k0 + B); // exactly the blocks up to the job's last: one read further is a report
        for (Blk &b : blocks) {
            b.rle_len = 1 + (uint32_t)below(below(2) ? 899999 : 50);
            b.in_len = b.rle_len + below(below(4) ? 1000 : (uint64_t)1 << 33); // a block of one long run: far more input than RLE1 bytes
        }
        const BzeSums s = bze_job_sums(blocks.data(), k0, B);
        uint32_t nmax = 0;
        uint64_t ntotal = 0, raw = 0;
        for (size_t k = k0; k < k0 + B; k++) {
            nmax = blocks[k].rle_len > nmax ? blocks[k].rle_len : nmax;
            ntotal += blocks[k].rle_len;
            raw += blocks[k].in_len;
        }
        CHECK(s.nmax == nmax && s.mmax == nmax + 1 && s.ntotal == ntotal && s.raw == raw, "blocks [%zu, +%u): nmax %u mmax %u ntotal %llu raw %llu", k0,
              B, s.nmax, s.mmax, (unsigned long long)s.ntotal, (unsigned long long)s.raw);
    }
}

// ---- the words zeroed before a pack, on a word array ---------------------------------------------------------------
// Words [0, count): up to the one behind the last word a bit of [0, end_bit) lands in -- what a pack that ends at end_bit needs.
static uint64_t words_needed(uint64_t end_bit)
{
    uint64_t count = 0;
    for (uint64_t b = end_bit < 40 ? 0 : end_bit - 40; b < end_bit; b++) count = b / 32 + 1 > count ? b / 32 + 1 : count;
    return count + 1;
}

struct Words { // the output buffer of one call: exactly cap_words words
    std::vector<uint8_t> zeroed, written;
    uint64_t base_word;
    void zero(const BzeZero &z, const char *what)
    {
        for (uint64_t w = z.from; w < z.to; w++) {
            CHECK(w < zeroed.size(), "%s: word %llu of %zu zeroed", what, (unsigned long long)w, zeroed.size());
            CHECK(w >= base_word, "%s: word %llu, below the call's first word %llu, zeroed", what, (unsigned long long)w, (unsigned long long)base_word);
            CHECK(!written[w], "%s: word %llu zeroed after a bit was written into it", what, (unsigned long long)w);
            zeroed[w] = 1;
        }
    }
    void touch(uint64_t w, const char *what) const
    {
        CHECK(w < zeroed.size(), "%s: word %llu of %zu touched", what, (unsigned long long)w, zeroed.size());
        CHECK(w < base_word || zeroed[w], "%s: word %llu was never zeroed", what, (unsigned long long)w);
    }
    void bits(uint64_t at, uint64_t n, bool and_behind, const char *what)
    {
        for (uint64_t b = at; b < at + n; b++) {
            touch(b / 32, what);
            written[b / 32] = 1;
        }
        if (n && and_behind) touch((at + n - 1) / 32 + 1, what); // the pack kernels may touch (not write) the word behind the last
    }
};

static void zero_case(uint64_t bit_base, bool seed, const std::vector<uint64_t> &T, uint64_t cap_words)
{
    Words o;
    o.zeroed.assign(cap_words, 0);
    o.written.assign(cap_words, 0);
    o.base_word = bit_base / 32;
    uint64_t zeroed_upto = bit_base / 32, cur = 0;
    uint32_t seeds = 0;
    for (size_t j = 0; j < T.size(); j++) {
        const BzeZero z = bze_zero_batch(bit_base, cur, T[j], zeroed_upto, cap_words);
        const uint64_t need = words_needed(bit_base + cur + T[j]);
        CHECK(z.over == (need > cap_words), "batch %zu at bit %llu of %llu bits: %llu words needed of %llu, over = %d", j,
              (unsigned long long)(bit_base + cur), (unsigned long long)T[j], (unsigned long long)need, (unsigned long long)cap_words, (int)z.over);
        if (z.over) return; // the call fails: nothing more is written
        if (z.to > z.from) { // (what encode_range does with the span)
            o.zero(z, "batch");
            if (seed && z.from == bit_base / 32) {
                seeds++;
                o.written[z.from] = 1; // the bits below the phase
            }
            zeroed_upto = z.to;
        }
        o.bits(bit_base + cur, T[j], true, "batch");
        cur += T[j];
    }
    CHECK(seeds == (seed && !T.empty() ? 1u : 0u), "the seed word was placed %u times", seeds);
    // the footer behind the blocks, or behind nothing: the caller zeroed the four words of an empty stream itself
    const uint64_t end = bit_base + cur;
    if (T.empty()) {
        if (cap_words < bit_base / 32 + 3 || bit_base % 32) return; // (an empty stream starts at bit 32 of a buffer of 16 bytes or more)
        for (uint64_t w = 0; w < bit_base / 32 + 3; w++) o.zeroed[w] = 1;
    }
    const BzeZero z = bze_zero_footer(end, !T.empty(), cap_words);
    CHECK(z.over == (words_needed(end + 80) > cap_words), "footer at bit %llu: %llu words needed of %llu, over = %d", (unsigned long long)end,
          (unsigned long long)words_needed(end + 80), (unsigned long long)cap_words, (int)z.over);
    if (z.over) return;
    o.zero(z, "footer");
    o.bits(end, 80, false, "footer");
}

static void check_zero(size_t cases)
{
    const uint64_t edge[] = {0, 1, 31, 32, 33};
    for (size_t c = 0; c < cases; c++) {
        const uint64_t bit_base = below(3) * 32 + below(32);
        std::vector<uint64_t> T(below(7));
        uint64_t total = 0;
        for (uint64_t &t : T) total += t = below(3) ? below(200) : edge[below(5)];
        // room: anywhere from far too little to plenty, and often within a word of what the call needs
        const uint64_t need = words_needed(bit_base + total + 80);
        const uint64_t cap_words = below(2) ? need - 2 + below(5) : below(need + 4);
        zero_case(bit_base, bit_base % 32 != 0 && below(2), T, cap_words);
    }
    for (uint64_t phase = 0; phase < 32; phase++) // every phase, a batch that ends one bit before, on and behind a word edge
        for (uint64_t t : {31 - phase, 32 - phase, 33 - phase, (uint64_t)64 - phase})
            for (uint64_t slack = 0; slack < 3; slack++) {
                zero_case(phase, phase != 0, {t, 1, 0, 32}, words_needed(phase + t + 33 + 80) - 1 + slack);
                zero_case(phase, false, {t}, words_needed(phase + t) - 1 + slack);
            }
    zero_case(32, false, {}, 4); // the empty stream: "BZh9", footer, in 16 bytes -- the check asks for the word behind them too
    zero_case(32, false, {}, 5);
}

// ---- the inputs a batch of a many-streams call closes --------------------------------------------------------------
// blocks[i]: the blocks of input i (0: an empty one), in batches of `per`
static void many_case(const std::vector<uint32_t> &blocks, size_t per)
{
    const size_t count = blocks.size();
    std::vector<uint32_t> plan_input; // exactly one entry a block
    for (size_t i = 0; i < count; i++) plan_input.insert(plan_input.end(), blocks[i], (uint32_t)i);
    const size_t nb = plan_input.size();
    std::vector<uint32_t> copy(plan_input); // (its own allocation of exactly nb entries)
    std::vector<long> closed_by(count, -1);
    uint32_t cur = 0;
    long batch = 0;
    for (size_t k0 = 0; k0 < nb || (nb == 0 && batch == 0); k0 += per, batch++) {
        const uint32_t B = (uint32_t)(nb - k0 < per ? nb - k0 : per);
        const BzeMany d = bze_many_batch(nb ? copy.data() : nullptr, k0, B, nb, count, cur);
        CHECK(d.lo == cur && d.close_hi >= d.lo && d.close_hi <= count, "batch %ld: lo %u close_hi %u, %u inputs closed so far of %zu", batch, d.lo,
              d.close_hi, cur, count);
        CHECK(d.hi >= d.close_hi && d.hi <= d.close_hi + 1 && d.hi <= count, "batch %ld: close_hi %u hi %u of %zu", batch, d.close_hi, d.hi, count);
        for (uint32_t i = d.lo; i < d.close_hi; i++) closed_by[i] = batch; // (in order and once each: [lo, close_hi) start where the last ended)
        bool started = false;
        for (size_t k = 0; k < k0; k++) started |= plan_input[k] == d.lo;
        CHECK((d.lo_started != 0) == started && d.lo_started <= 1, "batch %ld: lo %u lo_started %u, blocks in an earlier batch: %d", batch, d.lo,
              d.lo_started, (int)started);
        for (size_t k = k0; k < k0 + B; k++)
            CHECK(plan_input[k] >= d.lo && plan_input[k] < d.hi, "batch %ld places inputs [%u, %u), block %zu is of input %u", batch, d.lo, d.hi, k,
                  plan_input[k]);
        cur = d.close_hi;
    }
    CHECK(cur == count, "%u of %zu inputs closed", cur, count);
    size_t k = 0;
    for (size_t i = 0; i < count; i++) {
        CHECK(closed_by[i] >= 0, "input %zu never closed", i);
        k += blocks[i];
        if (blocks[i]) CHECK(closed_by[i] == (long)((k - 1) / per), "input %zu ends in batch %zu, closed by batch %ld", i, (k - 1) / per, closed_by[i]);
    }
}

static void check_many(size_t cases)
{
    for (size_t c = 0; c < cases; c++) {
        std::vector<uint32_t> blocks(below(9));
        const uint64_t shape = below(6);
        for (size_t i = 0; i < blocks.size(); i++) {
            blocks[i] = below(3) ? 1 + (uint32_t)below(below(3) ? 2 : 7) : 0; // empty ones anywhere
            if (shape == 0 || (shape == 1 && i < 2) || (shape == 2 && i + 2 >= blocks.size()) || (shape == 3 && i == blocks.size() / 2)) blocks[i] = 0;
        } // (shape 0: all empty; 1: at the front; 2: at the end; 3: in the middle)
        many_case(blocks, 1 + below(5));
    }
    many_case({}, 2);
    many_case({0}, 2);
    many_case({0, 0, 3, 0, 1, 1, 0}, 2); // (the item of 3 blocks straddles two batches)
    many_case({5}, 2);
}

int main(int argc, char **argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: plan_host <seed> <cases>\n");
        return 2;
    }
    rng_state = strtoull(argv[1], nullptr, 10) * 0x9E3779B97F4A7C15ull + 1;
    const size_t cases = (size_t)strtoull(argv[2], nullptr, 10);
    check_split(cases);
    check_sums(cases);
    check_zero(cases);
    check_many(cases);
    printf("plan_host: %zu cases each of the job split, job sums, zero spans and many-streams batches held\n", cases);
    return 0;
}
