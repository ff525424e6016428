// batch.h -- the device arrays of one batch and their layout in a context's arena: geometry, `Batch`, the carver every workspace
// is cut with, layout_batch, the named views of borrowed arrays.  No HIP call: common.h includes this behind <hip/hip_runtime.h>,
// tests/workspace_host/layout_host.cpp compiles the same text with g++ -fsanitize=address,undefined (vector types stood in for below).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

#ifndef __HIPCC__ // a host-only program
struct uint2 { uint32_t x, y; };
struct alignas(16) uint4 { uint32_t x, y, z, w; };
struct alignas(16) int4 { int32_t x, y, z, w; };
#endif

// ---- geometry -----------------------------------------------------------------------------
// Every per-block device array uses one stride S (bytes/elements per bzip2 block), a multiple
// of the sort tile so tiles never straddle blocks.
constexpr int SORT_THREADS = 512;
constexpr int DB_STRIDE = 1280; // digit-base entries per block: up to 5 digits x 256 values
constexpr int SORT_ITEMS = 16;
constexpr int SORT_TILE = SORT_THREADS * SORT_ITEMS; // 8192 elements per workgroup (512 x 16: halves the look-back /
                                                     // scan overhead per element against 256 x 16, -7 % on the bench)
// The stride of blocks of at most M RLE1 bytes (layout_batch); the largest a context can have is a level-9 block's, M = 899,999.
constexpr uint32_t batch_stride(uint32_t M) { return (uint32_t)(((size_t)M + 1 + SORT_TILE - 1) / SORT_TILE * SORT_TILE); }
constexpr uint32_t RANK_RESOLVED = 0x80000000u;      // suffix is alone in its group
constexpr uint32_t RANK_EMITTED = 31u << 26;         // (with RANK_RESOLVED, less = 0) its byte of the last column has been written (chunk_finish)
constexpr int SUMMARY_WORDS = 24; // round summary: see round_begin (bwt.hip)
constexpr uint32_t GID_MAX = 4096;  // large groups of a block a round can number densely (12 key bits)
constexpr int RS_ROWS = 22;       // per-block rows of the suffix sort's round state (layout_batch)
constexpr uint32_t MS_BG_ROW = 65552, MS_LEVELS = 5, MS_SEG_SLOTS = 112, MS_SEG_ROW = 264, MS_UNIT_CAP = 4096, MS_ITEM_CAP = 224,
                   MS_CNT_WORDS = 48, MS_MIN_N = 131072; // (levels whose blocks stay below MS_MIN_N bytes keep the 8-pass path: no tables for them)
constexpr int MAX_ROUNDS = 30; // depth 8 doubles every round and ends at 2^20; < 31 keeps the rank words' round tags unique

struct BlockDesc { // device-side description of one planned block (mirrors bzh_block + restart info)
    uint64_t in_off;
    uint64_t in_len;
    uint32_t rle_len;
    uint32_t crc;
};

// Device arrays of one batch of B blocks.  Passed to kernels by value.
struct Batch {
    uint32_t B;       // blocks in this batch
    uint32_t S;       // stride (elements) between blocks in per-block arrays
    uint32_t TPB;     // sort tiles per block stride (S / SORT_TILE)
    uint32_t M;       // max RLE1 bytes per block (100000*level-1)
    uint8_t *rle;     // [B][S]  RLE1 output = BWT input
    uint32_t *n;      // [B]     RLE1 length per block
    uint8_t *bwt;     // [B][S]
    uint32_t *ptr;    // [B]
    uint8_t *hasbyte; // [B][256]
    // suffix sorting
    uint32_t *rank; // [B][S]
    uint32_t *sa;   // [B][S]
    uint32_t *headp; // [B][S] group rank by SA position (SWEEP rounds read it instead of gathering)
    uint2 *binned;   // [B][S] (rank word, suffix) pairs of the initial sort, binned by 4096-suffix window (rank_apply); memory of
                     //        its own since round 5: a block on the 8 passes leaves its SA order in sa / headp at the same time
    uint2 *listA;   // [B][S] sort elements (ping-pong of the radix passes; the big-group list between rounds)
    uint2 *listB;   // [B][S]
    uint2 *listC;   // [B][S] small-group (TAIL) list of the block
    uint2 *listD;   // [B][S] TAIL records of the round in flight
    uint32_t *hist; // [B][TPB][512]: 2 KiB per sort tile -- look-back status words (256 x u64) or refine digit rows
    uint32_t *dbase; // [B][DB_STRIDE] digit bases of the look-back passes
    uint32_t *dtot;  // [B][DB_STRIDE] digit totals of an ACTIVE round (5 digits x 256)
    uint8_t *flg;   // [B][S]
    int4 *tagg;     // [B][TPB] tile carries: last group start / last boundary before the tile, first boundary after it
    // Round state of the suffix sort, all [B] unless noted.  The rounds are driven from the device: round_begin
    // turns the counters of the round before into this round's work lists, the host only sizes the launches
    // from a summary it reads one round late.
    uint32_t *st_mode;  // 0: whole block on the radix path, SA-order enumeration (SWEEP); 1: groups routed by size (SPLIT)
    uint32_t *st_h;     // depth of the block's next round
    uint32_t *st_nbig;  // records in the big-group list (SPLIT) / unresolved suffixes (SWEEP)
    uint32_t *st_ntail; // records in the small-group list
    uint32_t *st_tdst;  // which of listC (0) / listD (1) receives the block's small-group records this round: the survivors of
                        // tail_round (which reads the other one) and what refine appends; a block whose small groups sit a
                        // round out keeps its list where it is (round_begin)
    uint32_t *c_big, *c_small, *c_tail, *c_prog; // produced by a round: list lengths, "some group was refined"
    uint32_t *c_nolist; // produced by a round: refine did not write the block's lists (SWEEP mode, mostly large groups)
    uint32_t *c_groups; // groups of the block after the initial sort (refine_one<init>; round_begin picks the first mode)
    uint32_t *chain;    // [B][4] near-periodic blocks: flags, period, leading tails (period_probe, bwt.hip)
    uint32_t *pshrink;  // [B][4] blocks sorted as eight of their periods: flags, period, the block's real length, periods kept (period_detect / period_expand)
    uint32_t *gateS, *gateA, *gateR, *gateT;     // this round: sorted-list length per path (0 = not on that path)
    uint32_t *actS, *actA, *actR, *actT, *actQ;  // this round: ids of the blocks on each path (Q: TAIL at depth x4)
    uint32_t *nlist;    // [8] lengths of those lists (S, A, R, T, Q)
    unsigned long long *stat_A; // [1] sum over rounds of the unresolved suffixes entering them
    uint32_t *errflag; // [1]
    // Numbers for the large groups of a round (bwt.hip): whoever writes a large group to a big list (chunk_finish,
    // refine_one, refine) draws a number for it -- one atomic add per GROUP -- and leaves number -> rank and rank -> number;
    // the big lists are then sorted on [number : 12][key2 : 20] in FOUR 8-bit passes instead of on [rank : 20][key2 : 20]
    // in five.  (The order of the groups among each other does not matter: only that a group's records meet.)
    uint16_t *gidof;   // [B][S]  number of the large group whose rank this is (written for the ranks of large groups only)
    uint32_t *grank;   // [2][B][GID_MAX] rank of every numbered group; [round & 1]: a round's refine_one reads one half
                       //         while it fills the other for the next round
    uint32_t *gcount;  // [B]     numbers drawn for the lists being written (round_begin clears it)
    uint32_t *gwide;   // [2]     [round & 1] != 0: some block ran out of numbers for that round: its lists are sorted on ranks
    // bucket-first initial sort (bwt_msd.h): 2-byte buckets, oversized buckets split level by level, every bucket
    // that fits a tile finished inside one workgroup
    uint32_t *ms_bgcur;  // [B][65536] bigram counts, then claim cursors of the partition
    uint32_t *ms_pool;   // bucket starts: [B][MS_BG_ROW] (2-byte buckets), then [MS_LEVELS][B][MS_SEG_SLOTS][MS_SEG_ROW]
    uint32_t *ms_segcur; // [MS_LEVELS][B][MS_SEG_SLOTS][256] digit counts of an oversized bucket, then claim cursors
    uint4 *ms_units;     // [B * MS_UNIT_CAP] work list of the finishing kernel
    uint4 *ms_segs;      // [MS_LEVELS + 1][B * MS_SEG_SLOTS] oversized buckets per level
    uint32_t *ms_items;  // [MS_LEVELS + 1][B * MS_ITEM_CAP] (oversized bucket, tile) pairs per level
    uint32_t *ms_cnt;    // [MS_CNT_WORDS + (MS_LEVELS + 7) * B] counters; behind the first MS_CNT_WORDS per block: units, slot counters
                         // of the levels, unit tickets, "holds a group that spans several units", tickets and tile counts of
                         // mid_sort, records | runs << 20 of the big list being written (two rows, by round parity); then
                         // [3][B][MS_UNIT_CAP] x 2 words: the runs of those lists (two halves) and the tiles mid_plan packs them
                         // into (bwt.hip: msc_* accessors)
    uint32_t *ms_np;     // [B] 1: the block takes the bucket-first path (its first doubling round has depth 7)
    uint32_t *ms_old, *ms_new; // [B] ids of the blocks on the 8-pass path / on the bucket-first path
    uint32_t *ms_bincur; // [B][256] rank binning: pairs already claimed in each 4096-suffix window
    // inverse BWT (the decoder's back end, bzh_unbwt)
    uint8_t *unbwt_out; // [B][S]  where unbwt_run / unbwt_small_run leave a block (inverse RLE1 and unbwt_compare read it)
    // MTF / RLE2 (they keep no array of their own per byte or per tile: the tiles' tables are views of the sort lists, below)
    uint16_t *syms;    // [B][S+64]
    uint32_t *m;       // [B]   symbol count incl. EOB
    uint32_t *freqs;   // [B][258]
    uint32_t *nsyms;   // [B]
    // Huffman
    uint32_t *tfreq;   // [B][3][258]
    uint8_t *lens;     // [B][3][258]
    uint8_t *lens2;    // [2][B][3][258] huff_build: what each half of a block's attempts found (huff_header picks)
    uint32_t *lfit;    // [2][B][3] the scaling exponent that half found to fit (0xFFFFFFFF: none)
    uint32_t *ntab;    // [B]
    uint32_t *codes;   // [B][258]  (len << 24 | word) for table 0
    uint8_t *hdr;      // [B][HDR_BYTES] per-block header bits (block header .. coding tables)
    uint32_t *hdrbits; // [B][4] bits of part A, selector count, bits of part B, payload bits
    uint64_t *bits;    // [B]   total bits of the block
    uint64_t *bitoff;  // [B+1] exclusive scan of bits
    uint32_t *packgate; // [1] pack_gate: 1 = the batch's bits fit the output (the pack kernels of a gated call write nothing otherwise)
    uint32_t *symbits; // [B][PT] per pack tile bit counts
    BlockDesc *desc;   // [B]
    const BlockDesc *pdesc; // [B] where the block CRCs are read from: the plan's descriptors of this batch (rle1_emit; the CRCs may
                            //     arrive there on a side stream while the batch is already being sorted) or `desc` itself (stage seams)
    // "fixed" Huffman mode only (bzh_set_mode) -- the default path never touches these
    uint32_t *fx_tfreq;  // [B][6][258]
    uint8_t *fx_lens;    // [B][6][258]
    uint32_t *fx_codes;  // [B][6][258] (len << 24 | word)
    uint8_t *fx_sel;     // [B][FX_SELMAX] table of every 50-symbol segment
    uint8_t *fx_selbits; // [B][FX_SELBYTES] selectors, MTF + unary coded, as a bit string
    uint8_t *fx_hdr;     // [B][FX_HDR_BYTES] block header .. selector count, then the delta-coded tables
};

constexpr uint32_t MTF_TILE = 2048;  // BWT bytes walked by one wavefront (twice that in batches of 64 blocks and more: mtf_run)
static inline uint32_t mtf_tile_bytes(uint32_t B) { return B >= 64u ? 2u * MTF_TILE : MTF_TILE; } // the tile of a batch of B blocks (mtf_run)
// RLE2 layout of one MTF tile (mtf_tile_last -> mtf_prefix -> mtf_walk_par; read back by sync_emit)
struct MtfTile {
    int first;    // position in the block of the tile's first run head, -1 if none
    int last;     // of its last one, -1 if none; after mtf_prefix: the last run head BEFORE the tile
    uint32_t cnt; // symbols the tile emits, not counting the zero-run digits in front of `first`
    uint32_t off; // after mtf_prefix: output offset of the tile
};
constexpr uint32_t HDR_BYTES = 4160; // 64 B block header/symbol map/counts + up to 3 delta-coded tables (< 25.6 kbit)
constexpr uint32_t PACK_TILE = 4096; // MTF symbols packed by one workgroup
constexpr uint32_t FX_TABLES = 6;         // lib/huffman.rs:319-326 allows 2..6 tables
constexpr uint32_t FX_HDR_A = 64;         // bytes reserved for the part before the selectors
constexpr uint32_t FX_HDR_BYTES = 64 + 6 * 1152; // + up to 6 delta-coded tables (<= 5 + 258 * 35 bits each)

// ---- the carver ---------------------------------------------------------------------------------------------------------
// Cuts 256-byte aligned arrays off a base address, one after the other.  With a null base it only measures (every take returns
// nullptr, on integer arithmetic): a workspace is sized by a measuring pass of the function that lays it out.
struct CarveSpan { size_t off, count, elem; }; // where a take landed, what was asked for
struct Carver {
    uintptr_t base;
    size_t off = 0;
    std::vector<CarveSpan> *log = nullptr; // (the layout test: every take, in order)
    explicit Carver(void *b) : base(reinterpret_cast<uintptr_t>(b)) {}
    template <typename T>
    T *take(size_t count)
    {
        const size_t at = off;
        off += (count * sizeof(T) + 255) / 256 * 256;
        if (log) log->push_back({at, count, sizeof(T)});
        return base ? reinterpret_cast<T *>(base + at) : nullptr;
    }
    template <typename T>
    void put(T *&dst, size_t count) { dst = take<T>(count); }
    size_t bytes() const { return off; }
};

// ---- views: arrays a later stage borrows ---------------------------------------------------------------------------------
// An array whose owner is done with it is lent to a stage that needs room of another type.  Each loan is one function here, which
// producer and consumer both call, and one row of batch_views: the bytes the borrower needs and the lender has (layout_batch checks).
typedef unsigned long long bzh_u64;
static inline bzh_u64 *list_words(uint2 *list) { return reinterpret_cast<bzh_u64 *>(list); } // listA..D, binned: a pair as one 64-bit sort element
static inline int32_t *mtf_tlast(const Batch &bt) { return reinterpret_cast<int32_t *>(bt.listA); } // [B][MT][256] last position of every byte value before a tile (mtf_run; sync_emit reads it)
static inline MtfTile *mtf_tiles(const Batch &bt) { return reinterpret_cast<MtfTile *>(bt.listB); } // [B][MT] RLE2 layout of the tiles (the same two)
static inline uint32_t *huff_ranges(const Batch &bt) { return reinterpret_cast<uint32_t *>(bt.tagg); } // [B][8] symbol ranges of a block's tables (huff_prepare)
static inline bzh_u64 *refine_carry(const Batch &bt) { return reinterpret_cast<bzh_u64 *>(bt.tagg); } // [B][TPB][2] carry status words of refine; GEN_GID's look-back words (gst)
static inline bzh_u64 *sort_look(const Batch &bt) { return reinterpret_cast<bzh_u64 *>(bt.hist); }    // [B][TPB][256] look-back status words of the radix passes; refine's compaction (cstat)
static inline uint32_t *init_digits(const Batch &bt) { return reinterpret_cast<uint32_t *>(bt.flg); } // [B] rows S / 4 words apart, [TPB][512] each: digit rows of the initial refinement
static inline uint32_t *sweep_clist(const Batch &bt) { return reinterpret_cast<uint32_t *>(bt.listD); } // [B][2S] tails of a near-periodic block (period_probe writes, the SWEEP passes read)

struct BatchView { const char *name, *lender; size_t need, have; }; // (bytes)
constexpr int BATCH_VIEWS = 8;
static inline void batch_views(uint32_t nb, uint32_t s, uint32_t tpb, BatchView v[BATCH_VIEWS])
{
    const size_t B = nb, S = s, TPB = tpb;
    const size_t MT = (S + MTF_TILE - 1) / MTF_TILE; // tiles of MTF_TILE bytes: the smaller tile of mtf_tile_bytes, the larger need
    const size_t list = B * S * sizeof(uint2), hist = B * TPB * 512 * 4, flg = B * S, tagg = B * TPB * sizeof(int4);
    v[0] = {"list_words", "listA..D, binned", B * S * 8, list}; // (this row and sort_look hold by construction: listed for the record)
    v[1] = {"mtf_tlast", "listA", B * MT * 256 * 4, list};
    v[2] = {"mtf_tiles", "listB", B * MT * sizeof(MtfTile), list};
    v[3] = {"huff_ranges", "tagg", B * 8 * 4, tagg};
    v[4] = {"refine_carry", "tagg", B * TPB * 2 * 8, tagg};
    v[5] = {"sort_look", "hist", B * TPB * 256 * 8, hist};
    v[6] = {"init_digits", "flg", ((B - 1) * (S / 4) + TPB * 512) * 4, flg};
    v[7] = {"sweep_clist", "listD", B * 2 * S * 4, list};
}

// ---- the layout ----------------------------------------------------------------------------------------------------------
// Lays the arrays of a batch of B blocks of at most M RLE1 bytes out at `base`; with base == nullptr only measures.  *misfit (if
// asked for): the first view that does not fit the array it borrows, nullptr when all fit.
static inline size_t layout_batch(Batch &bt, void *base, uint32_t B, uint32_t M, const char **misfit = nullptr, std::vector<CarveSpan> *log = nullptr)
{
    Carver c(base);
    c.log = log;
    bt.B = B;
    bt.M = M;
    bt.S = batch_stride(M);
    bt.TPB = bt.S / SORT_TILE;
    const size_t S = bt.S, NB = B;
    const size_t PT = (S + 64 + PACK_TILE - 1) / PACK_TILE;
    c.put(bt.rle, NB * S);
    c.put(bt.n, NB);
    c.put(bt.bwt, NB * S);
    c.put(bt.ptr, NB);
    c.put(bt.hasbyte, NB * 256);
    c.put(bt.rank, NB * S);
    c.put(bt.sa, NB * S);
    c.put(bt.headp, NB * S);
    c.put(bt.binned, NB * S);
    c.put(bt.listA, NB * S);
    c.put(bt.listB, NB * S);
    c.put(bt.listC, NB * S);
    c.put(bt.listD, NB * S);
    c.put(bt.hist, NB * 512 * bt.TPB);
    c.put(bt.dbase, NB * DB_STRIDE);
    c.put(bt.dtot, NB * DB_STRIDE);
    c.put(bt.flg, NB * S);
    c.put(bt.tagg, NB * bt.TPB);
    { // round state of the suffix sort: RS_ROWS words per block, contiguous (one launch clears it: its length is part of that launch).
        // Rows without a name: 17 is the sixth list (bwt.hip: actP), 20 is spare, as are the SUMMARY_WORDS words behind nlist
        const size_t oA = (RS_ROWS * NB + 8 + SUMMARY_WORDS + 1) & ~(size_t)1; // 64-bit counter: even word index
        uint32_t *rs = c.take<uint32_t>(oA + 4);
        uint32_t **f[RS_ROWS] = {&bt.st_mode, &bt.st_h, &bt.st_nbig, &bt.st_ntail, &bt.c_big, &bt.c_small, &bt.c_tail,
                                 &bt.c_prog, &bt.gateS, &bt.gateA, &bt.gateR, &bt.gateT, &bt.actS, &bt.actA, &bt.actR,
                                 &bt.actT, &bt.actQ, nullptr, &bt.c_nolist, &bt.c_groups, nullptr, &bt.st_tdst};
        for (int k = 0; k < RS_ROWS; k++)
            if (f[k]) *f[k] = rs ? rs + (size_t)k * NB : nullptr;
        bt.nlist = rs ? rs + RS_ROWS * NB : nullptr;
        bt.stat_A = rs ? reinterpret_cast<unsigned long long *>(rs + oA) : nullptr;
    }
    c.put(bt.chain, NB * 4);
    c.put(bt.pshrink, NB * 4);
    c.put(bt.errflag, 64);
    c.put(bt.gidof, NB * S);
    c.put(bt.grank, 2 * NB * GID_MAX);
    c.put(bt.gcount, NB);
    c.put(bt.gwide, 64);
    { // bucket-first initial sort (bwt_msd.h): only levels whose blocks can reach MS_MIN_N bytes ever use it
        const size_t MB = M >= MS_MIN_N ? NB : 0;
        c.put(bt.ms_bgcur, MB * 65536);
        c.put(bt.ms_pool, MB * MS_BG_ROW + (size_t)MS_LEVELS * MB * MS_SEG_SLOTS * MS_SEG_ROW);
        c.put(bt.ms_segcur, (size_t)MS_LEVELS * MB * MS_SEG_SLOTS * 256);
        c.put(bt.ms_units, MB * MS_UNIT_CAP);
        c.put(bt.ms_segs, (size_t)(MS_LEVELS + 1) * MB * MS_SEG_SLOTS);
        c.put(bt.ms_items, (size_t)(MS_LEVELS + 1) * MB * MS_ITEM_CAP);
        c.put(bt.ms_cnt, MS_CNT_WORDS + (size_t)(MS_LEVELS + 7) * NB + 2 + 6 * NB * MS_UNIT_CAP);
        c.put(bt.ms_np, NB);
        c.put(bt.ms_old, NB);
        c.put(bt.ms_new, NB);
        c.put(bt.ms_bincur, NB * 256);
    }
    c.put(bt.unbwt_out, NB * S);
    c.put(bt.syms, NB * (S + 64));
    c.put(bt.m, NB);
    c.put(bt.freqs, NB * 258);
    c.put(bt.nsyms, NB);
    c.put(bt.tfreq, NB * 3 * 258);
    c.put(bt.lens, NB * 3 * 258);
    c.put(bt.lens2, 2 * NB * 3 * 258);
    c.put(bt.lfit, 2 * NB * 3);
    c.put(bt.ntab, NB);
    c.put(bt.codes, NB * 258);
    c.put(bt.hdr, NB * HDR_BYTES);
    c.put(bt.hdrbits, NB * 4);
    c.put(bt.bits, NB);
    c.put(bt.bitoff, NB + 1);
    c.put(bt.packgate, 4);
    c.put(bt.symbits, NB * PT);
    c.put(bt.desc, NB);
    bt.pdesc = bt.desc; // (rle1_emit points it at the plan's descriptors of the batch)
    { // "fixed" Huffman mode (optional)
        const size_t selmax = (S + 64 + 49) / 50 + 2;
        c.put(bt.fx_tfreq, NB * FX_TABLES * 258);
        c.put(bt.fx_lens, NB * FX_TABLES * 258);
        c.put(bt.fx_codes, NB * FX_TABLES * 258);
        c.put(bt.fx_sel, NB * selmax);
        c.put(bt.fx_selbits, NB * (((selmax * 6 + 7) / 8 + 8 + 63) / 64 * 64));
        c.put(bt.fx_hdr, NB * FX_HDR_BYTES);
    }
    BatchView v[BATCH_VIEWS];
    batch_views(B, bt.S, bt.TPB, v);
    if (misfit) *misfit = nullptr;
    for (int k = BATCH_VIEWS - 1; misfit && k >= 0; k--)
        if (v[k].need > v[k].have) *misfit = v[k].name;
    return c.bytes();
}

// Blocks a batch the arena is laid out for when a call needs batches of `blocks` (ensure_arena): at least 8, then
// multiples of 16, so that a stream of growing batches does not reallocate every time; never more than max_batch.
static inline uint32_t arena_batch(uint32_t blocks, uint32_t max_batch)
{
    const uint32_t want = blocks > 8 ? (blocks + 15u) & ~15u : 8;
    return want < max_batch ? want : max_batch;
}
