// encode_plan.h -- the host arithmetic between the encoder's kernels: how a range of plan blocks is cut into jobs, what a job's
// blocks add up to, which output words are zeroed before which pack ORs its bits into them, which inputs a batch of a
// many-streams call opens and closes, and how the plan's two workspaces are laid out (rle1.hip).  No HIP types: api.hip's encode drivers call these, and tests/encode_host/plan_host.cpp
// compiles the same text with g++ -fsanitize=address,undefined and holds each against brute force.  An off-by-one here is a bit
// ORed into a word that was never zeroed, or that was zeroed after it was written.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

#include "batch.h" // BlockDesc, the carver

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

// ---- the plan's workspaces (rle1.hip) -------------------------------------------------------------------------------------
constexpr int RL_THREADS = 256;
constexpr int RL_ITEMS = 16;
constexpr uint32_t RL_TILE = RL_THREADS * RL_ITEMS; // 4096 input bytes per workgroup
constexpr uint32_t GRAN = 64;                       // bytes per granule = one wavefront of the splitter
constexpr uint32_t GRAN_PER_TILE = RL_TILE / GRAN;  // 64
constexpr uint32_t NONE32 = 0xFFFFFFFFu;

struct BlockAux { // per planned block: what the emit kernel needs about the run the block starts in
    uint64_t Ce;      // canonical offset at the end of that run
    uint32_t A;       // RLE1 bytes of that run's remainder (chunking restarted at in_off)
    uint32_t e_first; // end of that run
    uint32_t open;    // 1 = the cut could move if more input followed (streaming: not final yet)
    uint32_t pad;
};

struct PlanArrays {
    const uint8_t *in;
    uint64_t n;
    uint32_t ntiles;
    uint32_t ngran;
    uint32_t M;
    uint32_t maxblocks;
    uint32_t start;    // input offset the split begins at (a block start; 0 unless a sharded rank continues a chain)
    uint32_t stop;     // the split ends with the first block that starts at or after this offset (a sharded rank's range end)
    uint32_t *lrs;     // [ntiles]   last run start inside the tile (NONE32 if none); then exclusive prefix max
    uint32_t *frs;     // [ntiles+1] first run start inside the tile; then suffix min (frs[ntiles] = n)
    uint32_t *csum;    // [ntiles]   canonical bytes emitted by the tile
    uint64_t *tc;      // [ntiles+1] exclusive scan of csum
    uint32_t *cg;      // [ngran]
    uint32_t *rsg;     // [ngran]
    uint32_t *nrsg;    // [ngran+1]  nrsg[ngran] = n
    BlockDesc *blocks; // [maxblocks]
    BlockAux *aux;     // [maxblocks]
    uint32_t *nblocks; // [1]
};

struct PlanWs { // layout of ctx->plan_ws
    PlanArrays pa;
    uint32_t *crcacc;
    size_t bytes;
};

// (`extra`: block records beyond the bound of one stream -- a plan over many inputs may cut one more block per input)
static inline PlanWs plan_layout(void *base, uint64_t n, uint32_t M, uint32_t extra, std::vector<CarveSpan> *log = nullptr)
{
    PlanWs w{};
    const uint64_t ntiles = (n + RL_TILE - 1) / RL_TILE;
    const uint64_t ngran = ntiles * GRAN_PER_TILE;
    const uint64_t maxblocks = n / ((uint64_t)(M - 1) * 4 / 5) + 4 + extra;
    Carver c(base);
    c.log = log;
    w.pa.n = n;
    w.pa.M = M;
    w.pa.ntiles = (uint32_t)ntiles;
    w.pa.ngran = (uint32_t)ngran;
    w.pa.maxblocks = (uint32_t)maxblocks;
    c.put(w.pa.lrs, ntiles + 2);
    c.put(w.pa.frs, ntiles + 2);
    c.put(w.pa.csum, ntiles + 2);
    c.put(w.pa.tc, ntiles + 2);
    c.put(w.pa.cg, ngran + 2);
    c.put(w.pa.rsg, ngran + 2);
    c.put(w.pa.nrsg, ngran + 2);
    c.put(w.pa.blocks, maxblocks); // blocks | aux | nblocks stay consecutive: one copy brings them back (rle1_plan_split)
    c.put(w.pa.aux, maxblocks);
    c.put(w.pa.nblocks, 64);
    c.put(w.crcacc, maxblocks);
    w.bytes = c.bytes();
    return w;
}

struct ManyInput {
    uint32_t gs;   // first byte in the guarded buffer (its guard is at gs + len)
    uint32_t len;  // bytes of the input
    uint32_t slot; // first record slot of the input in the split's record area (room for len / ((M-1) 4/5) + 1 blocks)
    uint32_t cnt;  // blocks cut (plan_many_split); 0xFFFFFFFF: more than that room
};
struct ManyWs { // layout of ctx->many_ws: guarded buffer | inputs | split records | block -> input
    uint8_t *gbuf;  // [ng + 32] the inputs, one guard byte behind each
    ManyInput *tab; // [count]
    BlockDesc *sb;  // [slots] what every input's split cuts, at the input's first slot
    BlockAux *sa;   // [slots]
    uint32_t *binp; // [maxblocks] input of every block of the plan
    uint64_t ng, slots, maxblocks; // (the plan's bound: plan_layout with one extra block an input)
    size_t bytes;
};
static inline uint64_t many_slots(uint64_t len, uint32_t M) { return len ? len / ((M - 1u) * 4u / 5u) + 1 : 0; } // record slots of one input
static inline ManyWs many_layout(void *base, const size_t *lens, size_t count, uint32_t M, std::vector<CarveSpan> *log = nullptr)
{
    ManyWs w{};
    for (size_t k = 0; k < count; k++) {
        w.ng += lens[k];
        w.slots += many_slots(lens[k], M);
    }
    w.ng += count;
    w.maxblocks = w.ng / ((M - 1u) * 4u / 5u) + 4 + count;
    Carver c(base);
    c.log = log;
    c.put(w.gbuf, w.ng + 32);
    c.put(w.tab, count);
    c.put(w.sb, w.slots);
    c.put(w.sa, w.slots);
    c.put(w.binp, w.maxblocks);
    w.bytes = c.bytes();
    return w;
}
