// encode_plan.h -- the host arithmetic between the encoder's kernels: how a range of plan blocks is cut into jobs, what a job's
// blocks add up to, which output words are zeroed before which pack ORs its bits into them, and which inputs a batch of a
// many-streams call opens and closes.  No HIP types: api.hip's encode drivers call these, and tests/encode_host/plan_host.cpp
// compiles the same text with g++ -fsanitize=address,undefined and holds each against brute force.  An off-by-one here is a bit
// ORed into a word that was never zeroed, or that was zeroed after it was written.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

struct BzeSpan { // a job
    size_t k0;  // its first plan block
    uint32_t B; // its blocks
};
struct BzeSums { // of a job's blocks
    uint32_t nmax, mmax;  // the longest block's RLE1 bytes; the symbols a block may have: m <= n + 1 (lib/mtf.rs:36)
    uint64_t ntotal, raw; // RLE1 bytes, input bytes
};
struct BzeZero {
    bool over;         // the words needed exceed the capacity: nothing is zeroed or written
    uint64_t from, to; // words [from, to) are zeroed now (to <= from: none)
};
struct BzeMany {
    uint32_t lo, lo_started, close_hi, hi; // ManyBatch's fields of the same names (common.h)
};

// Blocks a job of nb blocks gets when a lane takes batches of lane_mb blocks and there are NL lanes: as few jobs as the batch
// size allows, one for every lane where there are blocks enough, all of about the same size.
static inline size_t bze_per(size_t nb, uint32_t lane_mb, size_t NL)
{
    if (nb == 0) return 0;
    size_t njobs = (nb + lane_mb - 1) / lane_mb;
    if (njobs < NL && nb >= NL) njobs = NL; // give every lane work
    return (nb + njobs - 1) / njobs;
}

// [b0, b1) in jobs of `per` blocks, the last one shorter.
static inline void bze_split(size_t b0, size_t b1, size_t per, std::vector<BzeSpan> &jobs)
{
    jobs.clear();
    for (size_t k0 = b0; k0 < b1; k0 += per) jobs.push_back({k0, (uint32_t)(b1 - k0 < per ? b1 - k0 : per)});
}

// What blocks [k0, k0 + B) of a plan add up to (Blk: bzh_block -- rle_len, in_len).
template <class Blk>
static inline BzeSums bze_job_sums(const Blk *blocks, size_t k0, uint32_t B)
{
    BzeSums s = {0, 0, 0, 0};
    for (uint32_t b = 0; b < B; b++) {
        if (blocks[k0 + b].rle_len > s.nmax) s.nmax = blocks[k0 + b].rle_len;
        s.ntotal += blocks[k0 + b].rle_len;
        s.raw += blocks[k0 + b].in_len;
    }
    s.mmax = s.nmax + 1;
    return s;
}

// A batch of T bits goes behind the `cur` bits a call has written from bit `bit_base` of its output on.  The pack kernels OR
// into every word a bit lands in and may touch the one behind the last, so words up to there must be zero: those below
// bit_base / 32 are the caller's, [bit_base / 32, zeroed_upto) were zeroed for the call's earlier batches.  The first batch of a
// call has from == bit_base / 32: a seed word (the bits a streaming pass owes to that word) goes there, behind the memset.
static inline BzeZero bze_zero_batch(uint64_t bit_base, uint64_t cur, uint64_t T, uint64_t zeroed_upto, uint64_t cap_words)
{
    const uint64_t need_upto = (bit_base + cur + T + 31) / 32 + 1;
    return {need_upto > cap_words, zeroed_upto, need_upto};
}

// The 80 footer bits at bit `end` of a stream whose blocks encode_range wrote (any_blocks) or that has none (the caller zeroed
// the four words of an empty stream itself): the footer may reach one word past what the last batch zeroed.
static inline BzeZero bze_zero_footer(uint64_t end, bool any_blocks, uint64_t cap_words)
{
    const uint64_t from = (end + 31) / 32 + (any_blocks ? 1 : 0), to = (end + 80 + 31) / 32 + 1;
    return {to > cap_words, any_blocks ? from : to, to};
}

// The inputs a batch of a many-streams call deals with: plan blocks [k0, k0 + B) of nb, plan_input[k] = the input of block k
// (ascending; inputs without a block are empty), `count` inputs, `cur` = the first input no earlier batch has closed.  The batch
// closes [cur, close_hi): the inputs whose last block it holds and the empty ones in front of them -- behind them too when it
// is the last batch -- and places [cur, hi), one more while its last input goes on in the next batch.  nb == 0: every input is
// empty, one call with B == 0 closes them all.
static inline BzeMany bze_many_batch(const uint32_t *plan_input, size_t k0, uint32_t B, size_t nb, size_t count, uint32_t cur)
{
    if (nb == 0) return {cur, 0u, (uint32_t)count, (uint32_t)count};
    const size_t kl = k0 + B - 1;
    const uint32_t il = plan_input[kl];
    const bool last = kl + 1 == nb, closes = last || plan_input[kl + 1] != il;
    const uint32_t close_hi = last ? (uint32_t)count : (closes ? il + 1 : il);
    return {cur, (k0 > 0 && plan_input[k0 - 1] == cur) ? 1u : 0u, close_hi, closes ? close_hi : il + 1};
}
