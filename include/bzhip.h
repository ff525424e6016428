/*
 * bzhip.h -- C ABI of libbzhip.so: an MI355X (gfx950) bzip2 block encoder that emits the
 * same bits as jgbyrne/banzai v0.3.1 -- and, since the reference only "(currently)" lacks one, a
 * decoder for what it, libbz2 and this library write (bzh_decode*, below the encode entry points).
 *
 * The reference has no FFI; its boundary is the crate's public functions and the private
 * per-stage functions.  Each entry point below names the reference
 * interface it replaces.  Conventions: plain pointers and sizes, caller-owned buffers, int
 * status (0 = ok, negative = bzh_status), nothing unwinds across the ABI.  A context is bound
 * to ONE GPU (one process per GPU) and is single-threaded; distinct contexts may run
 * concurrently.  Pointers named d_* are DEVICE pointers (HBM); all others are host pointers.
 * There is no CPU fallback: every entry point that computes fails with BZH_E_HIP when no
 * gfx950 device is usable.
 */
#ifndef BZHIP_H
#define BZHIP_H

#include <stddef.h>
#include <stdint.h>

#if defined(BZH_BUILD)
#define BZH_API __attribute__((visibility("default")))
#else
#define BZH_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bzh_ctx bzh_ctx;

typedef enum {
    BZH_OK = 0,
    BZH_E_ARG = -1,   /* bad argument (reference: assert!/panic!, lib/lib.rs:89) */
    BZH_E_NOMEM = -2, /* host or device allocation failed */
    BZH_E_HIP = -3,   /* HIP runtime error / no usable device */
    BZH_E_CAP = -4,   /* output buffer too small; *out_len holds the size needed where stated */
    BZH_E_STATE = -5, /* call sequence error (e.g. encode_range without a plan) */
    BZH_E_DATA = -6   /* the input is not a valid bzip2 stream; bzh_last_error says what and where */
} bzh_status;

/* One bzip2 block of a plan: which raw bytes it consumes and what RLE1 makes of them.
 * Mirrors `Rle { output, chk, raw, consumed }` (lib/rle.rs:94-99) minus the byte vectors. */
typedef struct {
    uint64_t in_off;  /* first raw byte of the block                                   */
    uint64_t in_len;  /* raw bytes consumed (Rle::consumed)                             */
    uint32_t rle_len; /* RLE1 output bytes, <= 100000*level-1 (lib/rle.rs:121)          */
    uint32_t crc;     /* CRC-32/BZIP2 of the raw bytes (Rle::chk, lib/crc32.rs:31-48)   */
} bzh_block;

/* Per-stage device timings (milliseconds, HIP events on the context's stream) and counters of
 * the last bzh_encode* / bzh_encode_range_device call; filled when profiling is enabled. */
typedef struct {
    double ms_plan, ms_rle1, ms_bwt, ms_mtf, ms_huff, ms_pack, ms_total;
    double ms_bwt_sort;           /* the global radix passes only (radix_scatter: the 8 passes of blocks that keep them and
                                   * the big-list passes of the rounds; text batches launch none since round 5 -- the
                                   * dominant kernel class is chunk_finish, see bzh_get_kernel_stats)               */
    uint64_t bwt_sort_launches;   /* radix scatter launches issued in ms_bwt_sort (incl. ones that find no work) */
    uint64_t bwt_sort_elems;      /* elements moved by those launches                           */
    uint64_t raw_bytes, rle_bytes, mtf_syms, out_bits;
    uint64_t bwt_rounds;          /* prefix-doubling rounds run (max over blocks)               */
    uint64_t bwt_active_sum;      /* sum over rounds and blocks of unresolved suffixes (A)      */
    uint32_t blocks, pad;
} bzh_stats;

/* ---- lifecycle -------------------------------------------------------------------------- */

/* Create a context on HIP device `device` for block size `level` (1..9; lib/lib.rs:89).
 * max_batch = bzip2 blocks processed per kernel batch (0 = default). */
BZH_API int bzh_create(bzh_ctx **ctx, int device, int level, int max_batch);
/* 1 if a device whose hipDeviceProp_t::gcnArchName is `gcn_arch_name` can run this library (gfx950 only;
 * e.g. "gfx950:sramecc+:xnack-"), else 0.  bzh_create applies it to the chosen device and fails with
 * BZH_E_HIP otherwise. */
BZH_API int bzh_arch_supported(const char *gcn_arch_name);
BZH_API void bzh_destroy(bzh_ctx *ctx);
BZH_API const char *bzh_strerror(int status);
BZH_API const char *bzh_last_error(const bzh_ctx *ctx); /* detail of the last failure on this ctx   */
BZH_API int bzh_set_stream(bzh_ctx *ctx, void *hip_stream); /* hipStream_t to launch on (default 0) */
BZH_API int bzh_set_profiling(bzh_ctx *ctx, int enabled);
/* Huffman stage behaviour.  BZH_MODE_REFERENCE (default): bit-identical to banzai 0.3.1, including its table
 * count rule (2 or 3 tables from the ALPHABET size, lib/huffman.rs:319-326) and the refinement loop that zeroes
 * the tables (lib/huffman.rs:402-409), after which every segment uses table 0.  BZH_MODE_FIXED (SURVEY.md 8f row
 * f4, opt-in, NOT bit-identical to the reference): 2..6 tables chosen from the number of symbols as libbz2 does,
 * four real refinement iterations, per-segment selectors.  Every stream is a valid bzip2 stream either way. */
enum { BZH_MODE_REFERENCE = 0, BZH_MODE_FIXED = 1 };
BZH_API int bzh_set_mode(bzh_ctx *ctx, int mode);
/* 1 (default): batches run one after the other on the context's stream.  2: two half-batch lanes on
 * internal streams and host threads.  Measured on the 100 MB headline (one batch split in two): 2 lanes are 3-5 % SLOWER
 * than 1 (round 5: 8.73-8.93 against 8.34-8.41 ms; the per-batch latency chains -- huff_build, the late doubling rounds -- are paid
 * twice and overlap less than they cost); kept for experiments only. */
BZH_API int bzh_set_lanes(bzh_ctx *ctx, int lanes);
BZH_API int bzh_get_stats(const bzh_ctx *ctx, bzh_stats *out);
/* Test hook: inject a fault into the next suffix sort of this context (kind 1: one tile of the first block never
 * publishes its look-back status; 0: none).  The call that runs into it returns an error status -- the waits of
 * the look-backs are bounded -- and the context stays usable.  Kind 2: the same fault, treated as the one a GPU
 * shared with other processes produces (a look-back of a small batch gives up): the sort runs again with every
 * block pinned to one XCD and the call succeeds.  No counterpart in the reference. */
BZH_API int bzh_debug_fault(bzh_ctx *ctx, int kind);

/* Per-kernel-class figures of the last whole-path call made with profiling on (bench.py's `roofline.kernels`):
 * HIP-event time of the class's launches on the context's stream, launches issued, and the ALGORITHMIC bytes they
 * moved (per-element figures in DESIGN.md section 4 x the element counts of the plan and the round summaries).
 * *count receives the number of classes; BZH_E_CAP if max is smaller.  The reference has no counterpart. */
typedef struct bzh_kstat {
    char name[48];
    double ms;
    uint64_t launches;
    uint64_t alg_bytes;
} bzh_kstat;
BZH_API int bzh_get_kernel_stats(const bzh_ctx *ctx, bzh_kstat *out, size_t max, size_t *count);

/* ---- whole path: replaces banzai::encode(reader, writer, level), lib/lib.rs:84-132 -------- */

/* Host buffers in and out (H2D + encode + D2H).  Produces the complete .bz2 stream for the
 * slice in[0..n) -- identical to encode() fed by a reader that yields the slice -- and
 * returns the bytes consumed (== n) in *consumed.  BZH_E_CAP if cap is too small. */
BZH_API int bzh_encode(bzh_ctx *ctx, const uint8_t *in, size_t n, uint8_t *out, size_t cap, size_t *out_len,
               size_t *consumed);

/* Same, input and output resident in HBM (the timed path of bench.py). */
BZH_API int bzh_encode_device(bzh_ctx *ctx, const void *d_in, size_t n, void *d_out, size_t cap, size_t *out_len,
                      size_t *consumed);

/* ---- many inputs, one stream each: N calls of banzai::encode in one pass -------------------- */

/* Inputs back to back in d_in (16-byte aligned); input k is lens[k] bytes.  Stream k -- bit-identical to bzh_encode of input k
 * alone, in either Huffman mode -- is written at d_out + out_offs[k] (host arrays out).  Streams are laid back to back:
 * out_offs[0] = 0, out_offs[k+1] = align4(out_offs[k] + out_lens[k]), padding bytes zero; an empty input gets the 14-byte empty
 * stream ("BZh" + level, footer magic, CRC 0).  d_out must be 4-byte aligned and hold the streams' words:
 * cap >= align4(out_offs[count-1] + out_lens[count-1]), which bzh_encode_many_bound never falls below; otherwise BZH_E_CAP
 * (known only once everything is encoded).  count == 0 succeeds and writes nothing.  BZH_E_ARG (with bzh_last_error) for a
 * misaligned d_in or d_out, a null pointer where lengths are non-zero, or inputs whose bytes plus one per input exceed
 * 0xFFFF0000 (the plan's 32-bit positions).  The call runs on ONE lane (bzh_set_lanes does not apply), joins a streaming pass
 * in flight like every entry point, and fills bzh_get_stats / bzh_get_kernel_stats as bzh_encode_device does.  After an
 * error the context stays usable. */
BZH_API int bzh_encode_many_device(bzh_ctx *ctx, const void *d_in, const size_t *lens, size_t count, void *d_out, size_t cap,
                                   size_t *out_offs, size_t *out_lens);
/* Host buffers: ins[k][0..lens[k]) in, the same layout in out (one H2D of all inputs, one pass, one D2H); cap >=
 * out_offs[count-1] + out_lens[count-1] (else BZH_E_CAP). */
BZH_API int bzh_encode_many(bzh_ctx *ctx, const uint8_t *const *ins, const size_t *lens, size_t count, uint8_t *out, size_t cap,
                            size_t *out_offs, size_t *out_lens);
/* Upper bound of the total output for these lengths at this level (pure host arithmetic; 0 for a bad level): per stream the
 * blocks' RLE1 bytes (5/4 of the input + 8 a block) x 2.2 bytes (17-bit codes + 6 selector bits per 50 symbols), 4,400 bytes of
 * header and tables a block, 14 bytes of frame, 3 of alignment. */
BZH_API size_t bzh_encode_many_bound(int level, const size_t *lens, size_t count);
/* Seam: the plan alone.  bzh_plan_blocks then lists every input's blocks in input order, in_off relative to d_in; for every
 * input they equal what bzh_rle1_split returns for that input alone (offsets shifted by where it starts). */
BZH_API int bzh_plan_many_device(bzh_ctx *ctx, const void *d_in, const size_t *lens, size_t count, size_t *nblocks);

/* ---- decode: the inverse of the whole path.  The reference has no counterpart (README.md:9) ---------- */

/* in[0..n) holds one or more complete bzip2 streams back to back, as `bzip2 -d` accepts: of any level up to the context's
 * (a higher one: BZH_E_ARG), by any encoder (libbz2: 2..6 tables and real selectors; this library in either Huffman mode;
 * banzai).  Concatenation is handled inside the call: a pbzip2 file is thousands of streams.  out receives the decoded bytes
 * of all streams, *out_len their count, *consumed the bytes of `in` that belong to the decoded streams.
 * Where the input ends: behind a stream's footer, remaining bytes that begin with "BZh1".."BZh9" ARE the next stream and its
 * errors are errors; any other bytes are foreign, and decoding stops there with BZH_OK and *consumed < n.  Not one decoded
 * stream is BZH_E_DATA.
 * BZH_E_CAP: the output does not fit.  The call still finishes sizing and reports the total needed in *out_len (known only
 * once every block is decoded, as for bzh_encode_many); out[0..cap) is then unspecified; repeat the call with that size.
 * BZH_E_DATA: bad magic, truncation, a field outside the format (selectors 1..32767, code lengths 1..20, an over-subscribed
 * code, origPtr >= nblock, more bytes than the level's block size, a block that ends in four equal bytes without the count
 * byte libbz2 insists on), a block or stream CRC mismatch, and a RANDOMISED block: no current encoder writes one (a bzip2
 * 0.9.0 feature), so they are refused, not decoded.  Every table of a block is built and checked up front: an over-subscribed
 * table is refused even where no selector names it; libbz2, which never checks a table, accepts that unused-table form.
 * bzh_last_error names the kind, the stream, the block and the bit
 * position.  Every read and write of the decode kernels is bounded by construction, so a damaged stream yields a status and
 * the context stays usable.  Like every entry point the call joins a streaming pass in flight, runs on the context's stream
 * and honours bzh_set_profiling. */
BZH_API int bzh_decode(bzh_ctx *ctx, const uint8_t *in, size_t n, uint8_t *out, size_t cap, size_t *out_len, size_t *consumed);
/* Same, input and output resident in HBM (d_out may be null when cap is 0: sizing only). */
BZH_API int bzh_decode_device(bzh_ctx *ctx, const void *d_in, size_t n, void *d_out, size_t cap, size_t *out_len,
                              size_t *consumed);

/* Stage timings (milliseconds, HIP events, filled when profiling is enabled) and counters of the last bzh_decode* call.  A struct
 * of its own: bzh_stats keeps its layout. */
typedef struct {
    double ms_scan, ms_entropy, ms_unbwt, ms_unrle, ms_crc, ms_total;
    uint64_t streams, blocks;      /* decoded */
    uint64_t candidates;           /* magics the scan found, at any bit alignment */
    uint64_t candidates_off_chain; /* of those: inside a block's payload or behind the end, dropped by the chain walk */
    uint64_t in_bytes, out_bytes;
} bzh_decode_stats;
BZH_API int bzh_get_decode_stats(const bzh_ctx *ctx, bzh_decode_stats *out);

/* ---- many inputs, one decode each: N calls of bzh_decode in one pass (the inverse of bzh_encode_many) ---------- */

/* Input k is d_in[in_offs[k] .. in_offs[k] + in_lens[k]) and is judged exactly as bzh_decode judges that slice alone: one or
 * more streams of any encoder, foreign bytes behind them tolerated, nothing outside the slice looked at.  The slices ascend and
 * do not overlap; gaps between them are allowed, so bzh_encode_many_device's out_offs / out_lens are valid in_offs / in_lens as
 * they stand (its padding is the gaps).  BZH_E_ARG for the call, with nothing launched: a slice that reaches past n, slices that
 * descend or overlap, a null array with count > 0 (consumed alone may be null), a null buffer where bytes are claimed.
 * status[k] is what bzh_decode of input k alone returns with ample room: BZH_OK, BZH_E_DATA (an empty slice included), or
 * BZH_E_ARG for a stream above the context's level.  A failed input does not touch the others: it gets out_lens[k] = 0, and
 * consumed[k] as bzh_decode reports it (the end of the last stream the walk had passed when the failure was found).
 * bzh_last_error holds the text of the first failed input, prefixed with its number, positions counted inside its slice.  The
 * call itself returns BZH_OK when it ran to the end, even if every input failed: the statuses say what happened.
 * Output: the decoded inputs lie back to back from out_offs[0] = 0, no padding: out_offs[k+1] = out_offs[k] + out_lens[k];
 * when every input decodes, d_out / out_lens are bzh_encode_many_device's d_in / lens.  An input that fails after some of its
 * blocks were placed may leave a gap of at most the bytes it had decoded: the gap's bytes are unspecified, its out_lens[k] is 0,
 * and out_offs[k+1] lies behind the gap.
 * BZH_E_CAP as for bzh_decode: the call finishes sizing, all of out_offs / out_lens / status are set, the room needed is
 * out_offs[count-1] + out_lens[count-1] (gaps included), d_out is unspecified, and repeating the call with that room succeeds.
 * cap == 0 with a null d_out is a sizing call; like bzh_decode's it checks no CRC (blocks behind the point where the output
 * stops fitting are sized, not verified).
 * One scan covers the whole buffer and a batch takes the candidates of many inputs together: 4,096 one-block inputs are a few
 * batches, not 4,096 calls.  Blocks of at most bzh_decode_many_small_max() bytes go through an inverse BWT that works in LDS,
 * one workgroup a block; larger ones through the transform bzh_decode uses.  count == 0 succeeds.  After any outcome the context
 * stays usable.  The call joins a streaming pass in flight, runs on the context's stream and honours bzh_set_profiling, like
 * every entry point; bzh_get_decode_stats is filled as for bzh_decode, summed over the inputs. */
BZH_API int bzh_decode_many_device(bzh_ctx *ctx, const void *d_in, size_t n, const size_t *in_offs, const size_t *in_lens, size_t count,
                                   void *d_out, size_t cap, size_t *out_offs, size_t *out_lens, int *status, size_t *consumed);
/* Host buffers: ins[k][0..lens[k]) in (one H2D of all inputs, laid back to back without gaps), the decoded inputs in out as
 * above (one D2H).  BZH_E_ARG also for a null ins[k] with lens[k] > 0. */
BZH_API int bzh_decode_many(bzh_ctx *ctx, const uint8_t *const *ins, const size_t *lens, size_t count, uint8_t *out, size_t cap,
                            size_t *out_offs, size_t *out_lens, int *status, size_t *consumed);
/* The largest block (bytes of its last column, i.e. behind RLE1) the LDS inverse BWT takes: pure host, no context. */
BZH_API size_t bzh_decode_many_small_max(void);

/* Counters of the last bzh_decode_many* call; ms_unbwt_small (milliseconds, HIP events) is filled when profiling is enabled and
 * is part of bzh_decode_stats::ms_unbwt. */
typedef struct {
    uint64_t inputs, inputs_failed;
    uint64_t streams, blocks; /* met on the chains of all inputs */
    uint64_t blocks_small;    /* of those: through the LDS inverse BWT */
    uint64_t batches;         /* entropy-stage launches */
    double ms_unbwt_small;
} bzh_decode_many_stats;
BZH_API int bzh_get_decode_many_stats(const bzh_ctx *ctx, bzh_decode_many_stats *out);

/* ---- recovery: every block of a damaged input that verifies, and a report of every one that does not ---------- */

/* bzh_decode is all or nothing for an input, bzh_decode_many for each of its inputs; this is per BLOCK (what bzip2recover is
 * for).  One report entry per block magic that is not another block's payload, in ascending bit_pos. */
typedef struct {
    uint64_t bit_pos;  /* of the block magic */
    uint64_t end_bit;  /* kept: first bit behind the block; lost: 0 */
    uint64_t out_off;  /* kept: where its bytes lie in out; lost: the running total there (where the hole falls) */
    uint32_t out_len;  /* kept: decoded bytes; lost: 0 */
    uint32_t crc;      /* stored block CRC (the 32 bits behind the magic; 0 if the input ends before them) */
    uint32_t kind;     /* 0 = kept; else why it is lost: BZH_LOST_TRUNC 2, _FORMAT 3, _BLOCK_CRC 4, _RANDOMISED 6 */
    uint32_t flags;    /* kept entries only: BZH_REC_* */
    uint64_t err_bit;  /* lost: where the failure was found; kept: 0 */
} bzh_recover_entry;   /* 48 bytes */

enum { BZH_LOST_TRUNC = 2, BZH_LOST_FORMAT = 3, BZH_LOST_BLOCK_CRC = 4, BZH_LOST_RANDOMISED = 6 };
enum { BZH_REC_JOINED = 1, BZH_REC_STREAM_END = 2, BZH_REC_STREAM_OK = 4 };

/* The rules:
 * 1. Candidates.  The candidates are the block magics of the scan (bzh_decode_scan), at any bit alignment, ascending.  A magic
 *    of either kind that lies inside [bit_pos, end_bit) of the most recent KEPT block is that block's payload: it gets no entry
 *    (bzh_recover_stats::shadowed counts it).  Every other block magic gets exactly one entry, kept or lost.  A false magic inside
 *    the bytes of a LOST block cannot be told from a real one -- where a lost block ends is not known -- and is reported as lost.
 * 2. Kept.  A block is kept when the entropy stage decodes it, it holds at most 100000 x the CONTEXT's level bytes (a stream
 *    header may be gone, so no stream's level is asked), it does not end in four equal bytes without a count, and the CRC of its
 *    decoded bytes equals the stored one.  Otherwise it is lost, `kind` naming the first of these checks that failed (a truncated
 *    or malformed field or a RANDOMISED block: what the entropy stage says; too large or the open run: FORMAT).  Nothing about its
 *    neighbours decides this: a block is kept even if no magic follows it -- the entropy stage knows where a block ends by itself,
 *    so the block in front of a damaged magic is kept, which a split at the next magic would lose.
 * 3. Output.  The kept blocks' bytes lie back to back in out, in ascending order, no gaps: out_off is the running sum.  A lost
 *    block writes nothing anywhere.
 * 4. Verdict before placement.  Every clean candidate's CRC is folded from the bytes behind its inverse BWT with nothing
 *    written; only then are the kept blocks placed and expanded.  So cap == 0 with a null out is a complete verification run:
 *    *out_len is the exact size needed and the report is whole (the status is BZH_E_CAP unless nothing was kept).  BZH_E_CAP for
 *    a small out still returns every entry and *out_len (out is then unspecified); BZH_E_CAP for a small ent sets *count and
 *    *out_len (ent is then unspecified, out is written if it fits).
 * 5. Flags, on kept entries.  JOINED: the block starts 32 bits behind a stream header the walk accepts -- "BZh1".."BZh9" at
 *    byte 0 of the input, or the one an intact footer outside every kept block reports behind itself, as bzh_decode finds the
 *    next stream -- or it starts at the end_bit of the preceding entry and that entry is kept (the header, where both hold).
 *    STREAM_END: a footer magic lies at end_bit.  STREAM_OK, on a STREAM_END entry: that footer parses, the run of kept JOINED
 *    entries back from here reaches a stream header, every block of the run is within that header's level, and the fold of their
 *    stored CRCs equals the footer's -- the streams bzh_decode would accept alone.  streams_ok counts them, and the empty streams
 *    (an accepted header, an intact footer with CRC 0 right behind it), which have no entry.
 * 6. Status.  BZH_OK whenever the call ran to the end: no magic at all (*count == 0, *out_len == 0) and every block lost
 *    included -- the entries say what happened.  A stream above the context's level is not BZH_E_ARG here: its blocks that are
 *    too large are lost as FORMAT.  BZH_E_ARG: a null pointer where a size is claimed, a null out_len or count.
 * Not attempted: a second try at a kept block's end_bit when the magic there is damaged; RANDOMISED blocks (refused as by
 * bzh_decode, here reported as lost).  Like every entry point the call joins a streaming pass in flight, runs on the context's
 * stream, honours bzh_set_profiling and leaves the context usable after any outcome.  bzh_get_decode_stats: blocks = kept,
 * streams = streams_ok, candidates = all magics, candidates_off_chain = shadowed. */
BZH_API int bzh_recover_device(bzh_ctx *ctx, const void *d_in, size_t n, void *d_out, size_t cap, size_t *out_len,
                               bzh_recover_entry *ent, size_t max, size_t *count);
/* Same, host buffers in and out. */
BZH_API int bzh_recover(bzh_ctx *ctx, const uint8_t *in, size_t n, uint8_t *out, size_t cap, size_t *out_len,
                        bzh_recover_entry *ent, size_t max, size_t *count);

/* Counters of the last bzh_recover* call. */
typedef struct {
    uint64_t candidates; /* block magics the scan found */
    uint64_t kept, lost; /* entries */
    uint64_t shadowed;   /* magics of either kind inside a kept block */
    uint64_t footers;    /* footer magics outside every kept block */
    uint64_t streams_ok; /* rule 5 */
    uint64_t batches;    /* entropy-stage launches */
    uint64_t out_bytes;
} bzh_recover_stats;
BZH_API int bzh_get_recover_stats(const bzh_ctx *ctx, bzh_recover_stats *out);

/* The salvage as ONE valid .bz2 stream, built from the kept blocks' own bits: "BZh" + the context's level, the bits
 * [bit_pos, end_bit) of every kept entry (kind 0) concatenated in order, the footer magic, the fold of the entries' crc fields,
 * zero padding to a byte.  An archive stays an archive, and any bzip2 decoder can check the result.  in[0..n) is the input the
 * report was made from.  *out_len = 4 + ceil((sum of the kept entries' bits + 80) / 8) is pure arithmetic over the entries: it is
 * set before anything is launched, and on BZH_E_CAP too; with no kept entry the result is the 14-byte empty stream.  Every block
 * must be within the context's level for the stream to be valid: use the context the report was made with.
 * The entries are untrusted (they may come from a file) and are checked as a whole first.  BZH_E_ARG, with bzh_last_error naming
 * the entry: kept entries that do not ascend or that overlap, end_bit <= bit_pos + 80, end_bit > 8 n, a lost entry (kind != 0)
 * with a non-zero end_bit.  BZH_E_DATA, naming the entry: no block magic at a kept entry's bit_pos.  Lost entries are otherwise
 * ignored, and out_off / out_len / flags / err_bit of all.  No entry, whatever it holds, makes a kernel read outside in[0..n) or
 * write outside the words of *out_len.  The gather is one launch for all blocks (recover.hip).
 * Device variant: d_out must be 4-byte aligned (else BZH_E_ARG) and hold the stream's words, cap >= align4(*out_len), else
 * BZH_E_CAP; the bytes between *out_len and align4(*out_len) are written as zero.  Host variant: cap >= *out_len. */
BZH_API int bzh_recover_stream_device(bzh_ctx *ctx, const void *d_in, size_t n, const bzh_recover_entry *ent, size_t count,
                                      void *d_out, size_t cap, size_t *out_len);
BZH_API int bzh_recover_stream(bzh_ctx *ctx, const uint8_t *in, size_t n, const bzh_recover_entry *ent, size_t count,
                               uint8_t *out, size_t cap, size_t *out_len);

/* ---- random access: a verified block index, and the decode of a byte range of the output ---------- */

/* One decoded block.  bzip2 blocks are independent once the bit they start at is known: the index records that bit for every
 * block of every stream of an input, where its bytes lie in the concatenated output, and its stored CRC. */
typedef struct {
    uint64_t bit_pos;  /* of the block magic, in the coordinates of the input the index was built from */
    uint64_t end_bit;  /* first bit behind the block */
    uint64_t out_off;  /* of its first decoded byte in the concatenated output of all streams */
    uint32_t out_len;  /* decoded bytes */
    uint32_t crc;      /* stored block CRC */
    uint32_t stream;   /* 0-based stream number */
    uint32_t level;    /* of that stream, 1..9 */
} bzh_index_entry;     /* 40 bytes */

/* Builds the index of in[0..n): same input contract as bzh_decode (several streams, foreign bytes behind them, the level gate,
 * the error kinds).  Everything a full decode verifies is verified -- every block CRC and every stream CRC included -- without
 * an output buffer: a block's CRC is computed from the bytes behind its inverse BWT, its expansion is never written.  Empty
 * streams contribute no entry.  *count = entries (set also when max is too small: BZH_E_CAP, idx then unspecified), *out_total =
 * decoded bytes of all streams, *consumed as bzh_decode reports it (may be null).  idx may be null when max is 0. */
BZH_API int bzh_decode_index(bzh_ctx *ctx, const uint8_t *in, size_t n, bzh_index_entry *idx, size_t max, size_t *count,
                             uint64_t *out_total, size_t *consumed);
BZH_API int bzh_decode_index_device(bzh_ctx *ctx, const void *d_in, size_t n, bzh_index_entry *idx, size_t max, size_t *count,
                                    uint64_t *out_total, size_t *consumed);

/* Pure host arithmetic (no context, no GPU): the entries [*first, *last) that the output range [off, off + len) touches, the
 * range clipped to the indexed total, and the bytes [*byte_lo, *byte_hi) = [bit_pos / 8, ceil(end_bit / 8)) of the indexed input
 * that hold them.  An empty range (len 0, off at or behind the total, no entries) gives *first == *last and *byte_lo ==
 * *byte_hi.  The entries must be ordered as bzh_decode_index writes them.  BZH_E_ARG for a null pointer. */
BZH_API int bzh_index_span(const bzh_index_entry *idx, size_t count, uint64_t off, uint64_t len, size_t *first, size_t *last,
                           uint64_t *byte_lo, uint64_t *byte_hi);

/* Decodes output bytes [off, off + len) of the indexed input, clipped to its total: exactly min(len, total - off) bytes go to
 * out and *out_len (off >= total: none, BZH_OK).  in[0..n) holds the compressed bytes FROM BYTE in_byte_base of the indexed
 * input: all of it with base 0, or just the span bzh_index_span names.  Only the touched blocks are decoded -- no scan, no
 * walk along the chain -- and no decoded byte outside the range is written anywhere: whole blocks inside the range are
 * expanded in place, the at most two blocks at its edges are clipped to it.  The host variant uploads only the span.
 * BZH_E_ARG, with bzh_last_error naming the entry: an index that is not well formed (bit_pos not ascending, end_bit <= bit_pos,
 * out_off not the running sum from 0, a level outside 1..9 or above the context's), a buffer that does not cover the span, a
 * cap below the bytes to write; also for 2^32 entries or more.  BZH_E_DATA, naming the entry and the check, when a touched block does not match its entry: no
 * block magic at bit_pos, another end_bit, stored CRC or decoded size, more bytes than its level allows, an end in four equal
 * bytes without a count, a computed CRC that differs from the stored one.
 * WHAT IS VERIFIED: the CRC of every touched block, over all of its bytes.  Stream CRCs are NOT verified (they need every
 * block of the stream: bzh_decode_index has checked them), and damage in a block the range does not touch is not seen.
 * After any error the context stays usable.  bzh_get_decode_stats: blocks = blocks touched, candidates = 0. */
BZH_API int bzh_decode_range(bzh_ctx *ctx, const uint8_t *in, size_t n, uint64_t in_byte_base, const bzh_index_entry *idx,
                             size_t count, uint64_t off, uint64_t len, uint8_t *out, size_t cap, size_t *out_len);
/* Same, compressed bytes and output resident in HBM (idx is a host array). */
BZH_API int bzh_decode_range_device(bzh_ctx *ctx, const void *d_in, size_t n, uint64_t in_byte_base, const bzh_index_entry *idx,
                                    size_t count, uint64_t off, uint64_t len, void *d_out, size_t cap, size_t *out_len);

/* ---- sync points: states of the entropy stage inside a block, so that a read decodes its blocks in parallel segments ---- */

/* The entropy stage of a block is serial: the bit position, the Huffman table in use (it switches every 50 symbols, by the
 * block's selectors), the inverse MTF list and the RLE2 run accumulator all carry from symbol to symbol.  That state is small.
 * A sync point is that state at the boundary in front of group `group` of a block: with it the symbols from there on decode
 * without the ones before.  The index build walks every block once anyway and writes a point every `interval` groups; a range
 * decode then starts one wavefront per segment (from point to point) instead of one per block. */
typedef struct {
    uint64_t bit_pos;    /* of the first code of group `group`, in the coordinates of the indexed input */
    uint32_t entry;      /* the bzh_index_entry it belongs to */
    uint32_t group;      /* selector index of the first group decoded from here, 1 .. nsel-1 */
    uint32_t out_pos;    /* bytes of the block's last column written before it (a pending run NOT included) */
    uint32_t run;        /* RUNA/RUNB run accumulated so far, 0 = none */
    uint32_t run_weight; /* weight of the next run digit, 1 = none pending */
    uint32_t reserved;   /* 0 */
    uint8_t mtf[256];    /* the MTF list: the bytes in use in list order, then zeros */
} bzh_sync_point;        /* 288 bytes */

/* bzh_decode_index that also writes the sync points: one in front of every group whose selector index is a multiple of
 * `interval` (1..32767, else BZH_E_ARG), ordered by (entry, group).  The state behind a block's header (group 0) is not stored,
 * every decode parses the header anyway; a block of fewer groups than the interval has no point.  The input contract, the
 * verification, the errors and idx / *count / *out_total / *consumed are bzh_decode_index's, and the entries are the same.
 * *count and *npts are both set on success and on BZH_E_CAP, which is returned when either array is too small (both are then
 * unspecified): size with one call, fill with a second.  idx may be null when max is 0, pts when max_pts is 0. */
BZH_API int bzh_decode_index_sync(bzh_ctx *ctx, const uint8_t *in, size_t n, uint32_t interval, bzh_index_entry *idx, size_t max,
                                  size_t *count, bzh_sync_point *pts, size_t max_pts, size_t *npts, uint64_t *out_total,
                                  size_t *consumed);
BZH_API int bzh_decode_index_sync_device(bzh_ctx *ctx, const void *d_in, size_t n, uint32_t interval, bzh_index_entry *idx,
                                         size_t max, size_t *count, bzh_sync_point *pts, size_t max_pts, size_t *npts,
                                         uint64_t *out_total, size_t *consumed);

/* bzh_decode_range with sync points: the same bytes, the same clipping, nothing written outside the range, the same checks of
 * every touched block against its entry, every touched block's CRC verified, stream CRCs not.  Only the entropy stage differs:
 * one wavefront parses each touched block's header, then one wavefront per segment decodes from its point to the next.
 * npts == 0 is bzh_decode_range.  The points are untrusted (they may come from a file) and are checked as a whole, whatever the
 * range, before anything is launched.  BZH_E_ARG, with bzh_last_error naming the point: (entry, group) not ascending, an entry
 * outside the index, group 0 or above 32766, reserved not 0, a bit_pos not strictly inside its entry or not ascending, an out_pos
 * that descends or exceeds the level's block size, a run / run_weight pair the decoder cannot be in (run_weight a power of two
 * up to 2^22, run + 1 in [run_weight, 2 run_weight - 1]).  A point that is well formed but wrong for the bytes is BZH_E_DATA
 * naming the entry and the point: every segment must arrive exactly at the next point's bit_pos, out_pos, run, run_weight and
 * MTF list, so each point is checked by the segment in front of it, and the first by the header; behind that stand the entry's
 * checks and the block CRC.  No point, whatever it holds, makes a kernel read or write outside its tables and its block's slot. */
BZH_API int bzh_decode_range_sync(bzh_ctx *ctx, const uint8_t *in, size_t n, uint64_t in_byte_base, const bzh_index_entry *idx,
                                  size_t count, const bzh_sync_point *pts, size_t npts, uint64_t off, uint64_t len, uint8_t *out,
                                  size_t cap, size_t *out_len);
BZH_API int bzh_decode_range_sync_device(bzh_ctx *ctx, const void *d_in, size_t n, uint64_t in_byte_base, const bzh_index_entry *idx,
                                         size_t count, const bzh_sync_point *pts, size_t npts, uint64_t off, uint64_t len,
                                         void *d_out, size_t cap, size_t *out_len);

/* ---- many ranges in one call: every touched block is decoded once, in shared batches ---------------------------------- */

/* Output bytes [off, off + len) of the indexed input.  off + len saturates: a range that would end behind 2^64 - 1 ends there. */
typedef struct {
    uint64_t off, len;
} bzh_range;

/* Pure host arithmetic (no context, no GPU): the entries the ranges touch -- the union over the ranges, ascending and unique,
 * as entry numbers in touched[0 .. *ntouched) --, the bytes [*byte_lo, *byte_hi) of the indexed input from the first touched
 * entry's bit_pos / 8 to the last one's ceil(end_bit / 8) (the hull: what lies between two touched entries is inside it), and
 * *out_total = the sum over the ranges of min(len, total - off).  Nothing touched: *ntouched = 0, *byte_lo == *byte_hi == 0.
 * *ntouched is set also when max is too small: BZH_E_CAP, touched then unspecified; touched may be null when max is 0.
 * BZH_E_ARG: a null pointer, 2^32 entries or more.  The entries must be ordered as bzh_decode_index writes them. */
BZH_API int bzh_index_spans(const bzh_index_entry *idx, size_t count, const bzh_range *ranges, size_t nranges, uint32_t *touched,
                            size_t max, size_t *ntouched, uint64_t *byte_lo, uint64_t *byte_hi, uint64_t *out_total);

/* bzh_decode_range_sync_device for nranges ranges at once.  A single-range read costs one block's serial entropy stage however
 * short it is; here all ranges share their batches, so N short reads cost about what one costs.
 * RANGES.  Each is clipped to the indexed total exactly as bzh_decode_range clips: out_lens[r] = min(len, total - off), 0 for
 * off >= total.  They come in any order and may overlap, nest, repeat and be empty.
 * OUTPUT.  The ranges' bytes lie back to back in d_out in the order given, no padding: out_offs[0] = 0, out_offs[r + 1] =
 * out_offs[r] + out_lens[r], *out_total their sum.  All three are pure arithmetic over idx and ranges: they are set before
 * anything is launched and on every error below except a null-pointer BZH_E_ARG.  cap < *out_total: BZH_E_CAP, nothing
 * launched.  No byte outside d_out[0, *out_total) is written.
 * ONE DECODE PER BLOCK.  The touched blocks are bzh_index_spans' list.  Each goes through the entropy stage, the inverse BWT
 * and the CRC exactly once per call, however many ranges want it: bzh_get_decode_stats().blocks == blocks_touched.  A block
 * that exactly one range wants whole and no other range touches is expanded in place (blocks_whole counts these); of every
 * other one the tiles are expanded once and copied to each piece -- the intersection of one range with one block -- that meets
 * them.
 * VERIFIED: every touched block against its entry as by bzh_decode_range (the magic, end_bit, the stored CRC, the size, the
 * level's block size, the open run of four), and its CRC over all of its bytes.  Stream CRCs are NOT verified, untouched blocks
 * not looked at.  BZH_E_DATA names the first failing entry in ascending order, in bzh_decode_range's words.  The call is all or
 * nothing: after an error d_out is unspecified; the context stays usable.
 * d_in[0..n) holds the compressed bytes from byte in_byte_base of the indexed input and must cover [byte_lo, byte_hi) of
 * bzh_index_spans, else BZH_E_ARG.  npts == 0: one wavefront a block; otherwise the points are checked as a whole and every
 * touched block is decoded in segments, as by bzh_decode_range_sync.  The index is checked as a whole first, whatever the
 * ranges (BZH_E_ARG as bzh_decode_range; also for 2^32 entries or more).  nranges == 0 or nothing touched: BZH_OK, *out_total =
 * 0.  Like every entry point the call joins a streaming pass in flight, runs on the context's stream and honours
 * bzh_set_profiling.  idx, pts, ranges, out_offs and out_lens are host arrays. */
BZH_API int bzh_decode_ranges_device(bzh_ctx *ctx, const void *d_in, size_t n, uint64_t in_byte_base, const bzh_index_entry *idx,
                                     size_t count, const bzh_sync_point *pts, size_t npts, const bzh_range *ranges, size_t nranges,
                                     void *d_out, size_t cap, size_t *out_offs, size_t *out_lens, size_t *out_total);
/* Same, host buffers.  Only [byte_lo, byte_hi) goes up (a buffer that does not cover it goes up whole: the device call says what
 * is missing); sparse reads over a large input should hand in the touched blocks' bytes alone, with a sub-index. */
BZH_API int bzh_decode_ranges(bzh_ctx *ctx, const uint8_t *in, size_t n, uint64_t in_byte_base, const bzh_index_entry *idx,
                              size_t count, const bzh_sync_point *pts, size_t npts, const bzh_range *ranges, size_t nranges,
                              uint8_t *out, size_t cap, size_t *out_offs, size_t *out_lens, size_t *out_total);

/* Counters of the last bzh_decode_ranges* call. */
typedef struct {
    uint64_t ranges;         /* given */
    uint64_t pieces;         /* (range, block) pairs that meet */
    uint64_t blocks_touched; /* bzh_index_spans' list */
    uint64_t blocks_whole;   /* of those: expanded in place */
    uint64_t batches;        /* entropy-stage launches */
} bzh_decode_ranges_stats;
BZH_API int bzh_get_decode_ranges_stats(const bzh_ctx *ctx, bzh_decode_ranges_stats *out);

/* ---- records: a table of delimiter counts beside the index, and reads by record number ------------------------------------ */

/* DEFINITIONS.  `delim` is one byte value, `total` the indexed output's size, D the number of delimiter bytes in the output,
 * numbered 1..D by position p_1 < .. < p_D.  Record r, 0 <= r <= D, is the bytes [s_r, e_r) with s_0 = 0, s_r = p_r + 1,
 * e_r = p_(r+1) + 1 for r < D and e_D = total: the delimiter belongs to the record it ends, and record D is the unterminated
 * tail, which may be empty.  nrecords = D + (total > 0 && the last byte != delim): the records a reader of lines counts.
 * THE RECORD TABLE is uint64_t rec_cum[count + 1] beside an index of `count` entries: rec_cum[e] = the delimiters in output
 * bytes [0, idx[e].out_off), rec_cum[count] = D.
 * A RANGE OF RECORDS is a bzh_range {off = first record, len = number of records}: the bytes [s_off, s_(off+len)), with
 * s_k = total for k > D; off + len saturates.  It is clipped to the D + 1 records there are. */

/* bzh_decode_index_sync that also fills the record table and *nrecords.  interval 0: entries only (*npts = 0).  The input
 * contract, the verification, the errors, idx / *count, pts / *npts, *out_total and *consumed are byte for byte those of
 * bzh_decode_index_sync.  The delimiters are counted from the bytes behind each block's inverse BWT where its CRC is folded:
 * nothing is expanded, nothing more is waited for.  BZH_E_CAP also when max_cum < *count + 1 (*count is set). */
BZH_API int bzh_decode_index_records(bzh_ctx *ctx, const uint8_t *in, size_t n, uint32_t interval, uint8_t delim,
                                     bzh_index_entry *idx, size_t max, size_t *count, bzh_sync_point *pts, size_t max_pts,
                                     size_t *npts, uint64_t *rec_cum, size_t max_cum, uint64_t *nrecords, uint64_t *out_total,
                                     size_t *consumed);
BZH_API int bzh_decode_index_records_device(bzh_ctx *ctx, const void *d_in, size_t n, uint32_t interval, uint8_t delim,
                                            bzh_index_entry *idx, size_t max, size_t *count, bzh_sync_point *pts,
                                            size_t max_pts, size_t *npts, uint64_t *rec_cum, size_t max_cum,
                                            uint64_t *nrecords, uint64_t *out_total, size_t *consumed);

/* The same table from the decoded bytes d_raw[0..n) (device memory) and an index of them: after bzh_encode_index_device the
 * encoder's input is at hand, and the table costs one pass over it at memory bandwidth instead of a decode.  rec_cum holds
 * count + 1 words (host).  BZH_E_ARG: an index that is not well formed (as bzh_decode_range), or whose total is not n. */
BZH_API int bzh_count_records_device(bzh_ctx *ctx, const void *d_raw, size_t n, uint8_t delim, const bzh_index_entry *idx,
                                     size_t count, uint64_t *rec_cum, uint64_t *nrecords);

/* Pure host arithmetic (no context, no GPU), in the style of bzh_index_spans: the entries a read of these ranges of records
 * must decode -- ascending and unique -- and the hull [*byte_lo, *byte_hi) of their compressed bytes.  A range touches the block
 * that holds delimiter `off` (entry 0 for off == 0), the block that holds delimiter `off + len` (the last entry when that
 * exceeds D), and every block between them.  A BLOCK WHOSE LAST BYTE IS THE BOUNDARY DELIMITER IS TOUCHED ALTHOUGH IT GIVES THE
 * RANGE NO BYTES: the table says which block holds the delimiter, only the decode says where in it.  A range that is empty after
 * clipping (len 0, off > D) touches nothing.  The ranges need not ascend here.  *ntouched is set also when max is too small
 * (BZH_E_CAP).  BZH_E_ARG: a null pointer, 2^32 entries or more, a table that is not well formed (see below). */
BZH_API int bzh_record_spans(const bzh_index_entry *idx, size_t count, const uint64_t *rec_cum, const bzh_range *ranges,
                             size_t nranges, uint32_t *touched, size_t max, size_t *ntouched, uint64_t *byte_lo,
                             uint64_t *byte_hi);

/* Reads ranges of records: only the touched blocks (bzh_record_spans' list) are decoded, once each, the boundary delimiters are
 * located on the device, and exactly the records' bytes go to d_out.
 * RANGES are in records, clipped as above.  They must ascend and must not overlap: after clipping, ranges[r + 1].off >=
 * ranges[r].off + ranges[r].len, else BZH_E_ARG naming the range.  Adjacent and empty ranges are allowed.  Because they ascend,
 * one pass over the touched blocks in ascending batches places everything: no block goes through the entropy stage twice.
 * OUTPUT.  The records' bytes lie back to back in range order: out_offs[r], out_lens[r] and *out_total are set on success and
 * on BZH_E_CAP.  When cap is too small the call stops emitting, goes on locating, and returns BZH_E_CAP with *out_total the room
 * needed (d_out is then unspecified), as bzh_decode does.  No byte outside d_out[0, *out_total) is written, and whole blocks
 * are not expanded into scratch.
 * VERIFIED: everything bzh_decode_ranges verifies -- every touched block against its entry, its CRC over all of its bytes, the
 * sync points (npts == 0: one wavefront a block) -- and, for every touched block, the table: the delimiters counted in the block
 * must be rec_cum[e + 1] - rec_cum[e], else BZH_E_DATA "record table does not match entry e".  The table is untrusted and is
 * checked as a whole first: rec_cum[0] == 0, ascending, no difference above its entry's out_len, else BZH_E_ARG.  The index and
 * the points are checked as by bzh_decode_ranges.  After any error the context stays usable.
 * bzh_get_decode_stats and bzh_get_decode_ranges_stats are filled as by bzh_decode_ranges: ranges, pieces, blocks_touched,
 * blocks_whole and batches keep their meanings.  A batch costs at most one wait more than bzh_decode_ranges pays.
 * d_in[0..n) holds the compressed bytes from byte in_byte_base of the indexed input and must cover bzh_record_spans' hull. */
BZH_API int bzh_decode_records_device(bzh_ctx *ctx, const void *d_in, size_t n, uint64_t in_byte_base,
                                      const bzh_index_entry *idx, size_t count, const bzh_sync_point *pts, size_t npts,
                                      const uint64_t *rec_cum, uint8_t delim, const bzh_range *ranges, size_t nranges, void *d_out,
                                      size_t cap, size_t *out_offs, size_t *out_lens, size_t *out_total);
/* Same, host buffers.  Only the hull goes up (a buffer that does not cover it goes up whole: the device call says what is
 * missing). */
BZH_API int bzh_decode_records(bzh_ctx *ctx, const uint8_t *in, size_t n, uint64_t in_byte_base, const bzh_index_entry *idx,
                               size_t count, const bzh_sync_point *pts, size_t npts, const uint64_t *rec_cum, uint8_t delim,
                               const bzh_range *ranges, size_t nranges, uint8_t *out, size_t cap, size_t *out_offs,
                               size_t *out_lens, size_t *out_total);

/* ---- search: the offsets and record numbers of every occurrence of a byte string, found on the device --------------------- */

/* The decoded bytes exist in HBM at the moment they are verified; a search over them is one streaming pass at memory speed beside
 * an entropy stage that is nine tenths of a decode.  These calls leave the bytes on the device and return only the hits.
 * CONTRACT, for every call below.  A hit is an output offset o with out[o .. o + plen) == pat[0 .. plen).  Every occurrence is a
 * hit, overlapping ones included: "aa" in "aaaa" has three hits.  Hits are reported in ascending off.  With BZH_SEARCH_RECORDS,
 * `record` is the number of `delim` bytes in output [0, off): by the definitions above, the record that holds byte off; a match
 * that spans a delimiter belongs to the record of its first byte.  Without the flag, record is 0.
 * *nhits is always the exact number of hits.  If it exceeds max the status is BZH_E_CAP and hits[0 .. max) hold the first max hits:
 * the call goes on counting, as bzh_decode goes on sizing.  max == 0 with null hits is a counting call and returns BZH_OK.
 * BZH_E_ARG: plen == 0, plen > BZH_SEARCH_MAX_PATTERN, a flag bit that is not defined, a null pat or nhits, a null hits with
 * max > 0.  A pattern longer than the output has no hits.  After any error hits is unspecified and the context stays usable.
 * Like every entry point the calls join a streaming pass in flight, run on the context's stream and honour bzh_set_profiling.
 * hits is a host array. */
typedef struct {
    uint64_t off;    /* of the match's first byte in the output */
    uint64_t record; /* BZH_SEARCH_RECORDS: the delimiters in front of it; else 0 */
} bzh_hit;           /* 16 bytes */
enum { BZH_SEARCH_RECORDS = 1 };
#define BZH_SEARCH_MAX_PATTERN 256

/* Searches decoded bytes that already lie in HBM -- the encoder's input, a decoder's output: the seam the kernel is tested
 * through.  d_raw must be 16-byte aligned, else BZH_E_ARG; any n, 0 included.  No read goes past d_raw[0, n) rounded up to the
 * aligned 4-byte word that holds byte n - 1. */
BZH_API int bzh_search_raw_device(bzh_ctx *ctx, const void *d_raw, size_t n, const uint8_t *pat, size_t plen, unsigned flags,
                                  uint8_t delim, bzh_hit *hits, size_t max, size_t *nhits);

/* Searches the output of in[0..n) without an output buffer.  The input contract is bzh_decode's, word for word: several streams,
 * foreign bytes behind them, the level gate, every error kind, and bzh_last_error's text.  Everything a full decode verifies is
 * verified, block and stream CRCs included.  The output searched is the concatenation of all streams: a match may span a block
 * boundary or a stream boundary.  *out_total = the decoded bytes, *consumed as bzh_decode reports it (either may be null).  The
 * call is all or nothing: a stream CRC is known only at the footer, so no hit is trusted until the call returns BZH_OK or
 * BZH_E_CAP.  Every batch is expanded into a staging buffer of the context's, which grows to the batch, and searched there behind
 * its CRC checks: at most one host wait a batch beyond what the decode pays.  bzh_get_decode_stats is filled as by bzh_decode. */
BZH_API int bzh_search_device(bzh_ctx *ctx, const void *d_in, size_t n, const uint8_t *pat, size_t plen, unsigned flags, uint8_t delim,
                              bzh_hit *hits, size_t max, size_t *nhits, uint64_t *out_total, size_t *consumed);
BZH_API int bzh_search(bzh_ctx *ctx, const uint8_t *in, size_t n, const uint8_t *pat, size_t plen, unsigned flags, uint8_t delim,
                       bzh_hit *hits, size_t max, size_t *nhits, uint64_t *out_total, size_t *consumed);

/* Finds the hits that lie wholly inside output [off, off + len) of the indexed input, clipped to the indexed total as
 * bzh_decode_range clips.  in[0..n) holds the compressed bytes from byte in_byte_base of the indexed input.  Only the entries
 * bzh_index_span names are decoded, each once, as WHOLE blocks into staging, in windows of consecutive entries up to the staging
 * target; the range is applied by the search, not by the expansion.  The index and the points are checked as by bzh_decode_ranges;
 * every touched block is checked against its entry, with its CRC over all of its bytes; stream CRCs are not checked, as there.
 * npts == 0: one wavefront a block.  With BZH_SEARCH_RECORDS rec_cum is required, else BZH_E_ARG; it is checked whole for shape as
 * bzh_decode_records checks it, supplies the delimiters in front of the first touched block, and every touched block's counted
 * delimiters must equal rec_cum[e + 1] - rec_cum[e], else BZH_E_DATA "record table does not match entry e".  Without the flag
 * rec_cum is not looked at.  The host variant uploads only the span.  bzh_get_decode_stats is filled as by bzh_decode_range. */
BZH_API int bzh_search_range_device(bzh_ctx *ctx, const void *d_in, size_t n, uint64_t in_byte_base, const bzh_index_entry *idx,
                                    size_t count, const bzh_sync_point *pts, size_t npts, const uint64_t *rec_cum, uint64_t off,
                                    uint64_t len, const uint8_t *pat, size_t plen, unsigned flags, uint8_t delim, bzh_hit *hits,
                                    size_t max, size_t *nhits);
BZH_API int bzh_search_range(bzh_ctx *ctx, const uint8_t *in, size_t n, uint64_t in_byte_base, const bzh_index_entry *idx, size_t count,
                             const bzh_sync_point *pts, size_t npts, const uint64_t *rec_cum, uint64_t off, uint64_t len,
                             const uint8_t *pat, size_t plen, unsigned flags, uint8_t delim, bzh_hit *hits, size_t max, size_t *nhits);

/* The staging target of the range search: 0 = the default, 128 MiB (the stream decoder's staging default); a non-zero value below
 * 1024: BZH_E_ARG.  A window always holds whole blocks and at least one block. */
BZH_API int bzh_search_set_room(bzh_ctx *ctx, size_t bytes);

/* Counters of the last bzh_search* call. */
typedef struct {
    uint64_t hits;         /* found (*nhits) */
    uint64_t windows;      /* searched: one for raw bytes, one a batch of a full search, the range search's windows */
    uint64_t tiles;        /* of 4,096 bytes, over all windows (the counting pass) */
    uint64_t staging_peak; /* bytes of the staging buffer */
} bzh_search_stats;
BZH_API int bzh_get_search_stats(const bzh_ctx *ctx, bzh_search_stats *out);

/* ---- grep: the records that hold a byte string, compacted on the device into the caller's buffer -------------------------- */

/* A search returns offsets; what is wanted is the line.  A verified batch lies expanded in the search's staging buffer with every
 * hit and every delimiter known: selecting the records that hold a hit and compacting their bytes are two more streaming passes
 * over bytes that are already there, beside an entropy stage that is nine tenths of a decode.
 * CONTRACT, for every call below.  Records are those of the records section: the delimiter belongs to the record it ends, the
 * unterminated tail is the last record, an empty tail is not a record, nrecords = delimiters + (total > 0 && last byte != delim).
 * A record is HIT when a match of pat starts inside it: a match that spans a delimiter belongs to the record of its first byte, and
 * a pattern may contain the delimiter.  A record is SELECTED when it is hit, or with BZH_GREP_INVERT when it is not.
 * OUTPUT.  The selected records' bytes lie back to back in out, in ascending record order, each with its delimiter; a selected
 * tail comes as it is.  ent[k] describes the k-th selected record: `record` its number (the number bzh_decode_records takes), `off`
 * its first byte's offset in the decoded output, `len` its length, `out_off` where it lies in out, the running sum of len.
 * COUNTS AND ROOM.  *nrecs (selected records) and *out_total (their bytes) are always exact.  An array that is null with zero room
 * is not asked for and never causes BZH_E_CAP; all of out, cap, ent, max null or zero is a counting call and returns BZH_OK.
 * Room that is asked for and too small gives BZH_E_CAP: the call goes on counting, out and ent are then unspecified, and
 * repeating the call with the exact room succeeds.
 * BZH_E_ARG: plen == 0, plen > BZH_SEARCH_MAX_PATTERN, a flag bit that is not defined, a null pat, nrecs or out_total, a null
 * array with room claimed; in the device variants a d_out that is not 4-byte aligned.
 * BOUNDS.  No read goes past the aligned 4-byte word that holds byte n - 1 of a text; no store goes outside out[0, *out_total),
 * ent[0, *nrecs) and the kernel's own tables.  Every workgroup copies only bytes of its own tile of 4,096: the cost of a call
 * does not depend on the lengths of the records.
 * Like every entry point the calls join a streaming pass in flight, run on the context's stream, honour bzh_set_profiling and
 * leave the context usable after any outcome.  ent is a host array; out is a device buffer in the _device variants. */
typedef struct {
    uint64_t record;  /* the record's number, from 0 */
    uint64_t off;     /* of its first byte in the decoded output */
    uint64_t len;     /* its bytes, the delimiter included */
    uint64_t out_off; /* of its first byte in out */
} bzh_grep_entry;     /* 32 bytes */
enum { BZH_GREP_INVERT = 1 };

/* Greps decoded bytes that already lie in HBM: the seam the kernel is tested through.  d_raw must be 16-byte aligned, else
 * BZH_E_ARG; any n, 0 included. */
BZH_API int bzh_grep_raw_device(bzh_ctx *ctx, const void *d_raw, size_t n, const uint8_t *pat, size_t plen, unsigned flags, uint8_t delim,
                                void *d_out, size_t cap, bzh_grep_entry *ent, size_t max, size_t *nrecs, uint64_t *out_total);

/* Greps the output of in[0..n).  The input contract, every check and every error text are bzh_decode's; block and stream CRCs are
 * verified.  The call is all or nothing: on any error out is unspecified.  *decoded_total = the decoded bytes, *consumed as
 * bzh_decode reports it (either may be null).  Every batch is expanded into the search's staging buffer behind the open record,
 * which is carried from batch to batch: an input without any delimiter holds all of its output in the carry.  One host wait a
 * batch beyond what the decode pays.  bzh_get_decode_stats is filled as by bzh_decode. */
BZH_API int bzh_grep_device(bzh_ctx *ctx, const void *d_in, size_t n, const uint8_t *pat, size_t plen, unsigned flags, uint8_t delim,
                            void *d_out, size_t cap, bzh_grep_entry *ent, size_t max, size_t *nrecs, uint64_t *out_total,
                            uint64_t *decoded_total, size_t *consumed);
BZH_API int bzh_grep(bzh_ctx *ctx, const uint8_t *in, size_t n, const uint8_t *pat, size_t plen, unsigned flags, uint8_t delim,
                     uint8_t *out, size_t cap, bzh_grep_entry *ent, size_t max, size_t *nrecs, uint64_t *out_total,
                     uint64_t *decoded_total, size_t *consumed);

/* Greps the whole indexed input through the indexed front, in windows of whole blocks up to the staging target
 * (bzh_search_set_room), as bzh_search_range walks them.  in[0..n) holds the whole indexed input.  The index and the points are
 * checked as by bzh_decode_ranges; every block is checked against its entry, with its CRC over all of its bytes; stream CRCs are
 * not checked, as there.  npts == 0: one wavefront a block.  It needs no record table: the whole file is walked, so record numbers
 * count from 0. */
BZH_API int bzh_grep_index_device(bzh_ctx *ctx, const void *d_in, size_t n, const bzh_index_entry *idx, size_t count,
                                  const bzh_sync_point *pts, size_t npts, const uint8_t *pat, size_t plen, unsigned flags, uint8_t delim,
                                  void *d_out, size_t cap, bzh_grep_entry *ent, size_t max, size_t *nrecs, uint64_t *out_total);
BZH_API int bzh_grep_index(bzh_ctx *ctx, const uint8_t *in, size_t n, const bzh_index_entry *idx, size_t count,
                           const bzh_sync_point *pts, size_t npts, const uint8_t *pat, size_t plen, unsigned flags, uint8_t delim,
                           uint8_t *out, size_t cap, bzh_grep_entry *ent, size_t max, size_t *nrecs, uint64_t *out_total);

/* Counters of the last bzh_grep* call. */
typedef struct {
    uint64_t records;      /* of the output (nrecords) */
    uint64_t selected;     /* of them (*nrecs) */
    uint64_t out_bytes;    /* their bytes (*out_total) */
    uint64_t windows;      /* one for raw bytes, one a batch, the indexed walk's windows; one more where bytes were held back */
    uint64_t tiles;        /* of 4,096 bytes, over all windows (the counting pass) */
    uint64_t carry_peak;   /* bytes of the longest carry: the open record and the last plen - 1 bytes */
    uint64_t staging_peak; /* bytes of the staging buffer */
} bzh_grep_stats;
BZH_API int bzh_get_grep_stats(const bzh_ctx *ctx, bzh_grep_stats *out);

/* CONTEXT RECORDS: grep -B before -A after.  A setting of the context, like bzh_set_mode: it stays until it is set again, the
 * default is 0, 0, and every bzh_grep* and bzh_grep_patset* call reads it when the call begins.  Any uint32_t value is valid.
 * THE RULE.  A record is PRIMARY when the contract above selects it.  Record r is SELECTED when some primary p has
 * p - before <= r <= p + after, clipped to the records that exist; the unterminated tail is a record like any other.  Every
 * selected record comes out once, in ascending order; overlapping and touching contexts merge.  A selected record that is not
 * primary is a CONTEXT RECORD: bit 63 of its entry's len is set (BZH_GREP_LEN_CONTEXT; never with 0, 0), the other bits are its
 * length, and out_off stays the running sum of the lengths.  A GROUP is a maximal run of consecutive selected record numbers.
 * Counts, rooms and bounds are the contract's, for the selected records, context records included.  With 0, 0 a call launches
 * exactly the kernels it launches without this setting.  Between two windows the closed records that a later primary may
 * still select -- at most `before` of them -- are carried with the open record; bzh_grep_stats.carry_peak counts their bytes. */
#define BZH_GREP_LEN_CONTEXT (1ull << 63)
BZH_API int bzh_grep_set_context(bzh_ctx *ctx, uint32_t before, uint32_t after);
/* Counters of the last bzh_grep* call, beside bzh_grep_stats.  With context 0, 0: matched = selected and the rest 0 (groups are
 * counted only when a context is set). */
typedef struct {
    uint64_t matched;      /* primary records: what grep -c prints */
    uint64_t context;      /* context records */
    uint64_t groups;       /* maximal runs of consecutive selected records */
    uint64_t pending_peak; /* the most records carried undecided from one window to the next */
} bzh_grep_context_stats;
BZH_API int bzh_get_grep_context_stats(const bzh_ctx *ctx, bzh_grep_context_stats *out);

/* ---- a set of patterns in one pass: grep -F -f FILE, -e A -e B, -i -------------------------------------------------------- */

/* A pattern set is compiled on the host into a byte-class map and a trie without failure links, and lies on its device from
 * bzh_patset_create on; every start position of the text walks the trie (PFAC).  count is 1..BZH_PATSET_MAX_PATTERNS, every
 * pattern 1..BZH_SEARCH_MAX_PATTERN bytes.  With BZH_PATSET_FOLD_ASCII the bytes 'A'..'Z' and 'a'..'z' compare equal; nothing
 * else folds.  Patterns that are equal after folding collapse into one, whose number is the lowest index among them.  The trie
 * may hold 65,535 states beyond its root; above that, and for a null array, a pattern of zero or too many bytes, an undefined
 * flag bit and count 0: BZH_E_ARG, bzh_last_error(ctx) names the figure.  The table is uploaded and waited for inside the call.
 * A set belongs to no context: it may be used with every context on the device of the one it was made with (on another device
 * the using call returns BZH_E_ARG) and may be destroyed before or after that context. */
typedef struct bzh_patset bzh_patset;
enum { BZH_PATSET_FOLD_ASCII = 1 };
#define BZH_PATSET_MAX_PATTERNS 65536
typedef struct {
    uint64_t patterns, distinct;   /* given / after folding and removing equals */
    uint32_t min_len, max_len;
    uint32_t states, classes;      /* rows (the root included) and columns of the table */
    uint64_t table_bytes;
} bzh_patset_info;
BZH_API int bzh_patset_create(bzh_ctx *ctx, const uint8_t *const *pats, const size_t *lens, size_t count, unsigned flags,
                              bzh_patset **out);
BZH_API void bzh_patset_destroy(bzh_patset *set); /* null allowed */
BZH_API int bzh_patset_get_info(const bzh_patset *set, bzh_patset_info *out);

/* A hit of a set is a pair (output offset, distinct pattern) with the pattern matching there: overlapping ones and several
 * patterns at one offset included ({"ab","abc"} in "abc": two hits).  Hits ascend by off, then by len.  `pattern` is the
 * pattern's number (see above), `record` as bzh_hit's. */
typedef struct {
    uint64_t off, record;
    uint32_t pattern, len;
} bzh_set_hit;       /* 24 bytes */

/* The single-pattern calls above with (pat, plen) replaced by a set: every other argument, the counting call, BZH_E_CAP and the
 * statistics are theirs word for word.  A range search reports the pairs with off >= the range's start and off + len <= its end.
 * A grep selects the records inside which a match of any pattern starts. */
BZH_API int bzh_search_patset_raw_device(bzh_ctx *ctx, const void *d_raw, size_t n, const bzh_patset *set, unsigned flags,
                                         uint8_t delim, bzh_set_hit *hits, size_t max, size_t *nhits);
BZH_API int bzh_search_patset_device(bzh_ctx *ctx, const void *d_in, size_t n, const bzh_patset *set, unsigned flags, uint8_t delim,
                                     bzh_set_hit *hits, size_t max, size_t *nhits, uint64_t *out_total, size_t *consumed);
BZH_API int bzh_search_patset(bzh_ctx *ctx, const uint8_t *in, size_t n, const bzh_patset *set, unsigned flags, uint8_t delim,
                              bzh_set_hit *hits, size_t max, size_t *nhits, uint64_t *out_total, size_t *consumed);
BZH_API int bzh_search_patset_range_device(bzh_ctx *ctx, const void *d_in, size_t n, uint64_t in_byte_base,
                                           const bzh_index_entry *idx, size_t count, const bzh_sync_point *pts, size_t npts,
                                           const uint64_t *rec_cum, uint64_t off, uint64_t len, const bzh_patset *set, unsigned flags,
                                           uint8_t delim, bzh_set_hit *hits, size_t max, size_t *nhits);
BZH_API int bzh_search_patset_range(bzh_ctx *ctx, const uint8_t *in, size_t n, uint64_t in_byte_base, const bzh_index_entry *idx,
                                    size_t count, const bzh_sync_point *pts, size_t npts, const uint64_t *rec_cum, uint64_t off,
                                    uint64_t len, const bzh_patset *set, unsigned flags, uint8_t delim, bzh_set_hit *hits, size_t max,
                                    size_t *nhits);
BZH_API int bzh_grep_patset_raw_device(bzh_ctx *ctx, const void *d_raw, size_t n, const bzh_patset *set, unsigned flags, uint8_t delim,
                                       void *d_out, size_t cap, bzh_grep_entry *ent, size_t max, size_t *nrecs, uint64_t *out_total);
BZH_API int bzh_grep_patset_device(bzh_ctx *ctx, const void *d_in, size_t n, const bzh_patset *set, unsigned flags, uint8_t delim,
                                   void *d_out, size_t cap, bzh_grep_entry *ent, size_t max, size_t *nrecs, uint64_t *out_total,
                                   uint64_t *decoded_total, size_t *consumed);
BZH_API int bzh_grep_patset(bzh_ctx *ctx, const uint8_t *in, size_t n, const bzh_patset *set, unsigned flags, uint8_t delim,
                            uint8_t *out, size_t cap, bzh_grep_entry *ent, size_t max, size_t *nrecs, uint64_t *out_total,
                            uint64_t *decoded_total, size_t *consumed);
BZH_API int bzh_grep_patset_index_device(bzh_ctx *ctx, const void *d_in, size_t n, const bzh_index_entry *idx, size_t count,
                                         const bzh_sync_point *pts, size_t npts, const bzh_patset *set, unsigned flags, uint8_t delim,
                                         void *d_out, size_t cap, bzh_grep_entry *ent, size_t max, size_t *nrecs,
                                         uint64_t *out_total);
BZH_API int bzh_grep_patset_index(bzh_ctx *ctx, const uint8_t *in, size_t n, const bzh_index_entry *idx, size_t count,
                                  const bzh_sync_point *pts, size_t npts, const bzh_patset *set, unsigned flags, uint8_t delim,
                                  uint8_t *out, size_t cap, bzh_grep_entry *ent, size_t max, size_t *nrecs, uint64_t *out_total);

/* ---- regular expressions: grep -E, a DFA walked on the device ------------------------------------------------------------- */

/* 1..BZH_PATSET_MAX_PATTERNS expressions of 1..BZH_REGEX_MAX_EXPR bytes each are compiled on the host into ONE automaton for
 * their union -- a DFA anchored at its start, in the shape of a set's trie -- which every start position of the text walks.  The
 * syntax is a subset of Python's `re` on bytes: literal bytes; \\ \. \[ \] \( \) \| \* \+ \? \{ \} \^ \$ \- \/ \n \t \r \f \v \0
 * \xHH and a backslash in front of any other ASCII byte that is no letter or digit; \d \D \w \W \s \S (ASCII); `.` (any byte but 0x0A; any byte with BZH_REGEX_DOTALL); [...] and [^...] with ranges;
 * ( ) and (?: ), both plain grouping; | ; ? * + {m} {m,} {m,n}.  Anchors and \b (admitted by the _ex calls below), backreferences, lookaround, lazy and possessive
 * quantifiers, named groups, inline flags, a { that opens no well-formed bound, a bound above 256, an unbalanced bracket, an
 * expression that matches the empty string and one whose shortest match exceeds max_span are refused with BZH_E_ARG, the
 * message naming the expression's number and the byte.  So is an automaton above 65,536 NFA positions or 65,535 DFA states.
 * With BZH_REGEX_FOLD_ASCII 'A'..'Z' and 'a'..'z' compare equal, in literals and in classes (re.IGNORECASE on bytes).
 *
 * The result is a bzh_patset: every bzh_search_patset* and bzh_grep_patset* call takes it unchanged, bzh_patset_get_info fills
 * patterns = distinct = the number of expressions, bzh_patset_destroy frees it.  THE RULE: a hit is a start o at which some
 * expression matches out[o .. o + L) for some 1 <= L <= max_span (and o + L <= the end of the text or of the wanted range).  A
 * start yields exactly ONE bzh_set_hit: len is the LONGEST such L, pattern the lowest-numbered expression that matches exactly
 * that length.  Overlapping starts are all hits.  A match longer than max_span is not found; `unbounded` says that the
 * expressions have such matches.  BZH_REGEX_NO_LDS keeps the table out of LDS (in_lds 0): for measurements. */
enum { BZH_REGEX_FOLD_ASCII = 1, BZH_REGEX_DOTALL = 2, BZH_REGEX_NO_LDS = 4 };
#define BZH_REGEX_MAX_SPAN 256      /* = BZH_SEARCH_MAX_PATTERN: the tile's halo and the carry stay as they are */
#define BZH_REGEX_MAX_EXPR 4096
typedef struct {
    uint64_t expressions;
    uint32_t min_len, max_len;     /* the shortest match; min(the longest, max_span) */
    uint32_t states, classes;      /* rows (the root included) and columns of the table */
    uint32_t unbounded, in_lds;    /* some match may exceed max_span; every workgroup stages the table into LDS */
    uint64_t table_bytes;
} bzh_regex_info;    /* 40 bytes */
BZH_API int bzh_regex_create(bzh_ctx *ctx, const uint8_t *const *exprs, const size_t *lens, size_t count, unsigned flags,
                             uint32_t max_span /* 1..256, 0 = 256 */, bzh_patset **out);
BZH_API int bzh_regex_get_info(const bzh_patset *set, bzh_regex_info *out); /* BZH_E_ARG for a set of plain strings */
/* The compile alone: pure host, no context, no GPU.  BZH_OK and *info (null allowed), or BZH_E_ARG and the reason in
 * err[0 .. errn) (null allowed). */
BZH_API int bzh_regex_check(const uint8_t *const *exprs, const size_t *lens, size_t count, unsigned flags, uint32_t max_span,
                            bzh_regex_info *info, char *err, size_t errn);

/* ASSERTIONS.  The three calls above refuse every anchor and \b, as they always have.  The _ex calls take a SYNTAX word beside the
 * flags: BZH_REGEX_ASSERT admits ^ $ \A \Z \b \B anywhere in an expression (a$\n^b, foo\b bar, (^|,)x; \b inside a class stays
 * refused, and so does an assertion under a quantifier, as in Python).  ONE RULE on every route -- Python's `re` on bytes under
 * re.MULTILINE:
 *     ^    at output offset 0 of the whole decoded text, and behind every byte 0x0A
 *     $    at the end of the whole decoded text, and in front of every byte 0x0A
 *     \A   only at output offset 0            \Z   only at the end of the whole decoded text
 *     \b   one neighbour is in [0-9A-Za-z_] and the other is not; the text's two ends count as "not".  \B: the opposite
 * Line anchors are about 0x0A, as `.` is, whatever the `delim` of the call; folding does not change what a word byte is.  An
 * assertion consumes nothing: min_len, max_len, max_span and a hit's len count consumed bytes, and an expression that can match the
 * empty string (^, ^$, \b) stays refused.  A hit must lie in the wanted range; its assertions see the REAL neighbours, those outside
 * the range included, so the hits are the same whichever route reports them and whatever the window size.
 * BZH_REGEX_WORD matches every expression e as grep -w does: e, not preceded and not followed by a word byte -- Python's
 * (?<![0-9A-Za-z_])(?:e)(?![0-9A-Za-z_]), every length of e tried.  BZH_REGEX_LINE matches ^(?:e)$, as grep -x.  The two exclude
 * each other; either works without BZH_REGEX_ASSERT.
 * THE RANGE ROUTES.  An automaton that looks around (bzh_regex_look) needs the byte in front of the wanted range and the byte
 * behind it: bzh_search_patset_range* decode the blocks of [off - look_behind, off + len + look_ahead), clipped to the output, and
 * still report only the hits wholly inside [off, off + len).  The _device variant must be handed the compressed bytes of that
 * WIDENED span: bzh_index_span on the widened range. */
enum { BZH_REGEX_ASSERT = 1, BZH_REGEX_WORD = 2, BZH_REGEX_LINE = 4 };
typedef struct {
    uint32_t look_behind, look_ahead; /* 0 or 1: some assertion sees the byte in front of a start / behind a match */
    uint32_t contexts;                /* distinct start rows, 1..4 */
    uint32_t reserved;
} bzh_regex_look;    /* 16 bytes */
BZH_API int bzh_regex_create_ex(bzh_ctx *ctx, const uint8_t *const *exprs, const size_t *lens, size_t count, unsigned flags,
                                uint32_t max_span, unsigned syntax, bzh_patset **out);
BZH_API int bzh_regex_check_ex(const uint8_t *const *exprs, const size_t *lens, size_t count, unsigned flags, uint32_t max_span,
                               unsigned syntax, bzh_regex_info *info, bzh_regex_look *look, char *err, size_t errn);
BZH_API int bzh_regex_get_look(const bzh_patset *set, bzh_regex_look *out); /* BZH_E_ARG for a set of plain strings */

/* ---- the matched parts alone: grep -o, the non-overlapping leftmost-longest matches compacted on the device ---------------- */

/* A search reports every start, overlapping ones included; a grep returns whole records.  bzh_match* selects what grep -o prints
 * and returns only those bytes.
 * THE RULE, over the whole decoded output (not line by line; for a pattern that cannot match the delimiter the two are the same).
 * For a start s that holds a match, L(s) in 1..256 is the length of the LONGEST match there, assertions applied: plen for a byte
 * string, the longest of the start's patterns for a set, what a search reports as len for an automaton; ties go to the lowest
 * pattern number.  A cursor walks from 0: the next selected match is at the lowest s >= cursor that holds a match, and the cursor
 * becomes s + L(s).  "aa" in "aaaa" has three hits under bzh_search and two matches here.
 * OUTPUT.  The selected matches' bytes lie back to back in out, with no separator, in ascending off.  ent[k] describes the k-th
 * match: `off` its first byte's offset in the decoded output, `len` its length, `pattern` its pattern's number (0 for a byte
 * string), `out_off` where it lies in out, the running sum of len, `record` the number of delimiters in front of off with
 * BZH_MATCH_RECORDS and 0 without it: a match belongs to the record of its first byte.
 * COUNTS AND ROOM are a grep's: *nmatches and *out_total are always exact; an array that is null with zero room is not asked for;
 * all of out, cap, ent, max null or zero is a counting call; room that is asked for and too small gives BZH_E_CAP, the call goes
 * on counting, out and ent are then unspecified, and repeating the call with the exact room succeeds.
 * BZH_E_ARG: a grep's cases; BZH_GREP_INVERT has no meaning here and any flag bit but BZH_MATCH_RECORDS is undefined.  The context
 * setting of bzh_grep_set_context is not read.
 * BOUNDS.  No read goes past the aligned 4-byte word that holds byte n - 1 of a text; no store goes outside out[0, *out_total),
 * ent[0, *nmatches) and the kernels' own tables.  Every workgroup stores only entries and bytes of matches that start in its own
 * tile of 4,096; no thread follows the chain of matches beyond a tile, or beyond its chunk of the tiles' 256-entry maps.
 * A byte-range form does not exist: the selection inside a range depends on the text in front of it.  A maximum count (-m) is
 * the caller's: read the first entries. */
typedef struct {
    uint64_t off;     /* of the match's first byte in the decoded output */
    uint64_t record;  /* delimiters in front of off (BZH_MATCH_RECORDS), else 0 */
    uint32_t pattern; /* the pattern's number; 0 for a byte string */
    uint32_t len;     /* its bytes, 1..256 */
    uint64_t out_off; /* of its first byte in out */
} bzh_match_entry;    /* 32 bytes */
enum { BZH_MATCH_RECORDS = 1 };

/* The variants are a grep's, argument for argument: decoded bytes in HBM (d_raw 16-byte aligned), the full route (CRCs of blocks
 * and streams verified, all or nothing), the indexed route over the whole file (no record table needed). */
BZH_API int bzh_match_raw_device(bzh_ctx *ctx, const void *d_raw, size_t n, const uint8_t *pat, size_t plen, unsigned flags, uint8_t delim,
                                 void *d_out, size_t cap, bzh_match_entry *ent, size_t max, size_t *nmatches, uint64_t *out_total);
BZH_API int bzh_match_device(bzh_ctx *ctx, const void *d_in, size_t n, const uint8_t *pat, size_t plen, unsigned flags, uint8_t delim,
                             void *d_out, size_t cap, bzh_match_entry *ent, size_t max, size_t *nmatches, uint64_t *out_total,
                             uint64_t *decoded_total, size_t *consumed);
BZH_API int bzh_match(bzh_ctx *ctx, const uint8_t *in, size_t n, const uint8_t *pat, size_t plen, unsigned flags, uint8_t delim,
                      uint8_t *out, size_t cap, bzh_match_entry *ent, size_t max, size_t *nmatches, uint64_t *out_total,
                      uint64_t *decoded_total, size_t *consumed);
BZH_API int bzh_match_index_device(bzh_ctx *ctx, const void *d_in, size_t n, const bzh_index_entry *idx, size_t count,
                                   const bzh_sync_point *pts, size_t npts, const uint8_t *pat, size_t plen, unsigned flags, uint8_t delim,
                                   void *d_out, size_t cap, bzh_match_entry *ent, size_t max, size_t *nmatches, uint64_t *out_total);
BZH_API int bzh_match_index(bzh_ctx *ctx, const uint8_t *in, size_t n, const bzh_index_entry *idx, size_t count,
                            const bzh_sync_point *pts, size_t npts, const uint8_t *pat, size_t plen, unsigned flags, uint8_t delim,
                            uint8_t *out, size_t cap, bzh_match_entry *ent, size_t max, size_t *nmatches, uint64_t *out_total);
BZH_API int bzh_match_patset_raw_device(bzh_ctx *ctx, const void *d_raw, size_t n, const bzh_patset *set, unsigned flags, uint8_t delim,
                                        void *d_out, size_t cap, bzh_match_entry *ent, size_t max, size_t *nmatches, uint64_t *out_total);
BZH_API int bzh_match_patset_device(bzh_ctx *ctx, const void *d_in, size_t n, const bzh_patset *set, unsigned flags, uint8_t delim,
                                    void *d_out, size_t cap, bzh_match_entry *ent, size_t max, size_t *nmatches, uint64_t *out_total,
                                    uint64_t *decoded_total, size_t *consumed);
BZH_API int bzh_match_patset(bzh_ctx *ctx, const uint8_t *in, size_t n, const bzh_patset *set, unsigned flags, uint8_t delim,
                             uint8_t *out, size_t cap, bzh_match_entry *ent, size_t max, size_t *nmatches, uint64_t *out_total,
                             uint64_t *decoded_total, size_t *consumed);
BZH_API int bzh_match_patset_index_device(bzh_ctx *ctx, const void *d_in, size_t n, const bzh_index_entry *idx, size_t count,
                                          const bzh_sync_point *pts, size_t npts, const bzh_patset *set, unsigned flags, uint8_t delim,
                                          void *d_out, size_t cap, bzh_match_entry *ent, size_t max, size_t *nmatches, uint64_t *out_total);
BZH_API int bzh_match_patset_index(bzh_ctx *ctx, const uint8_t *in, size_t n, const bzh_index_entry *idx, size_t count,
                                   const bzh_sync_point *pts, size_t npts, const bzh_patset *set, unsigned flags, uint8_t delim,
                                   uint8_t *out, size_t cap, bzh_match_entry *ent, size_t max, size_t *nmatches, uint64_t *out_total);

/* Counters of the last bzh_match* call. */
typedef struct {
    uint64_t matches;       /* selected (*nmatches) */
    uint64_t out_bytes;     /* their bytes (*out_total) */
    uint64_t candidates;    /* starts at or behind their window's cursor that hold a match */
    uint64_t entered_tiles; /* tiles of 4,096 entered beyond their first byte: a selected match spans the edge in front */
    uint64_t open_tiles;    /* tiles whose map from entry to exit is not constant */
    uint64_t windows;       /* one for raw bytes, one a batch, the indexed walk's windows; one more where bytes were held back */
    uint64_t tiles;         /* over all windows */
    uint64_t carry_peak;    /* bytes of the longest carry */
    uint64_t staging_peak;  /* bytes of the staging buffer */
} bzh_match_stats;
BZH_API int bzh_get_match_stats(const bzh_ctx *ctx, bzh_match_stats *out);

/* ---- grep over many inputs in one pass: bzgrep PATTERN over a directory of .bz2 files ----------------------------------------- */

/* THE RULE.  For every input k the call returns exactly what bzh_grep returns for input k alone: bytes, entries, counts and
 * status.  The decoded inputs lie in one device buffer as many texts with walls between them:
 *   - a match starts and ends inside one input; text split across the end of input k and the start of input k + 1 is no match;
 *   - a non-empty tail without a delimiter is that input's last record; record numbers and `off` restart at 0 with every input;
 *   - an assertion sees an input's two ends as the text's edges (\A ^ at its offset 0, \Z $ at its end, \b against nothing there),
 *     whatever byte of a neighbour lies beside them in the buffer;
 *   - a damaged input fails alone, as in bzh_decode_many: items[k].status, zero counts, none of its bytes scanned.
 * OUTPUT.  The selected records of input 0, then of input 1, ...: their bytes back to back in out, their entries back to back in
 * ent.  Input k's entries begin at ent[sum of items[j].selected, j < k], its bytes at the out_off of its first entry; `record` and
 * `off` count from the input's start, `out_off` points into the call's out.  items[k] says what bzh_grep says of input k alone.
 * COUNTS AND ROOM as in the grep contract: *nrecs, *out_total and every item are always exact, a null array with zero room is not
 * asked for, all four null or zero is a counting call.  A room that is asked for and too small: nothing is gathered, BZH_E_CAP,
 * and repeating the call with the exact rooms succeeds.  The call itself returns BZH_OK when it ran to the end, even if every
 * input failed.
 * BZH_E_ARG: the grep's cases; a null offs, lens or items with count > 0; a context whose bzh_grep_set_context is not 0, 0
 * (context records over many inputs are not built); more than 2^31 - 1 virtual tiles (below).  count == 0 succeeds.  After any
 * outcome the context stays usable.
 * COST.  One workgroup per (input, 4,096-byte tile of the buffer that it meets): an input shorter than a tile still costs a tile's
 * work, and a tile that several inputs meet is read once per input.  No atomics; one host wait before the gather. */
typedef struct {
    uint64_t decoded;   /* the input's decoded bytes (a raw segment's length) */
    uint64_t records;   /* of them (nrecords) */
    uint64_t selected;  /* of those */
    uint64_t out_bytes; /* their bytes */
    int32_t status;     /* BZH_OK, or what bzh_decode_many says of the input */
    uint32_t reserved;  /* 0 */
} bzh_grep_many_item;   /* 40 bytes */

/* Texts that already lie in HBM, for instance bzh_decode_many_device's output: text k is d_raw[offs[k] .. offs[k] + lens[k]).
 * The seam the kernels are tested through.  d_raw must be 16-byte aligned and readable to the aligned 4-byte word that holds byte
 * n - 1, as for bzh_grep_raw_device.  The segments ascend and do not overlap; gaps are allowed and never scanned.  Anything else
 * is BZH_E_ARG naming the segment. */
BZH_API int bzh_grep_many_raw_device(bzh_ctx *ctx, const void *d_raw, size_t n, const size_t *offs, const size_t *lens, size_t count,
                                     const uint8_t *pat, size_t plen, unsigned flags, uint8_t delim, void *d_out, size_t cap,
                                     bzh_grep_entry *ent, size_t max, bzh_grep_many_item *items, size_t *nrecs, uint64_t *out_total);
/* Inputs as bzh_decode_many_device takes them, with its checks.  They are decoded into a staging buffer of the context, sized from
 * the compressed bytes; where that is too small the buffer is sized once more from the total the walk reports and the decode runs
 * again (bzh_grep_many_stats.staging_retries): the call never returns BZH_E_CAP for its own staging.  Then the one segmented pass. */
BZH_API int bzh_grep_many_device(bzh_ctx *ctx, const void *d_in, size_t n, const size_t *in_offs, const size_t *in_lens, size_t count,
                                 const uint8_t *pat, size_t plen, unsigned flags, uint8_t delim, void *d_out, size_t cap,
                                 bzh_grep_entry *ent, size_t max, bzh_grep_many_item *items, size_t *nrecs, uint64_t *out_total);
/* Host pointers as bzh_decode_many takes them: one H2D of all inputs, one D2H of the selected bytes (behind BZH_OK only). */
BZH_API int bzh_grep_many(bzh_ctx *ctx, const uint8_t *const *ins, const size_t *lens, size_t count, const uint8_t *pat, size_t plen,
                          unsigned flags, uint8_t delim, uint8_t *out, size_t cap, bzh_grep_entry *ent, size_t max,
                          bzh_grep_many_item *items, size_t *nrecs, uint64_t *out_total);
/* The same for a bzh_patset: a set of strings, or a regex with or without assertions. */
BZH_API int bzh_grep_many_patset_raw_device(bzh_ctx *ctx, const void *d_raw, size_t n, const size_t *offs, const size_t *lens, size_t count,
                                            const bzh_patset *set, unsigned flags, uint8_t delim, void *d_out, size_t cap,
                                            bzh_grep_entry *ent, size_t max, bzh_grep_many_item *items, size_t *nrecs, uint64_t *out_total);
BZH_API int bzh_grep_many_patset_device(bzh_ctx *ctx, const void *d_in, size_t n, const size_t *in_offs, const size_t *in_lens, size_t count,
                                        const bzh_patset *set, unsigned flags, uint8_t delim, void *d_out, size_t cap,
                                        bzh_grep_entry *ent, size_t max, bzh_grep_many_item *items, size_t *nrecs, uint64_t *out_total);
BZH_API int bzh_grep_many_patset(bzh_ctx *ctx, const uint8_t *const *ins, const size_t *lens, size_t count, const bzh_patset *set,
                                 unsigned flags, uint8_t delim, uint8_t *out, size_t cap, bzh_grep_entry *ent, size_t max,
                                 bzh_grep_many_item *items, size_t *nrecs, uint64_t *out_total);

/* Counters of the last bzh_grep_many* call (bzh_get_grep_stats is filled as well, summed over the inputs). */
typedef struct {
    uint64_t inputs, inputs_failed;
    uint64_t segments;        /* non-empty texts: those that own a virtual tile */
    uint64_t virtual_tiles;   /* workgroups of the counting pass */
    uint64_t shared_tiles;    /* tiles of the buffer that more than one segment meets */
    uint64_t staging_retries; /* 0 or 1: the decode ran again with the staging buffer sized from the walk's total */
} bzh_grep_many_stats;
BZH_API int bzh_get_grep_many_stats(const bzh_ctx *ctx, bzh_grep_many_stats *out);

/* ---- the encoder writes the index of its own stream: no decode pass to rediscover what it held -------------------------- */

/* bzh_encode_device that also returns the index of the stream it writes: the entries bzh_decode_index would return for
 * d_out[0..*out_len), and, with interval in 1..32767, the sync points bzh_decode_index_sync would return for that interval,
 * byte for byte (one in front of every group whose index is a positive multiple of interval, ordered by (entry, group), mtf =
 * the bytes in use in list order, then zeros, reserved 0).  interval 0: entries only (pts may be null, *npts = 0).  The stream
 * is bit-identical to bzh_encode_device's, in either Huffman mode.  An entry's bit_pos is 32 + the bits of the blocks before
 * it, its end_bit the next block's bit_pos (the last one's: the bit of the footer magic), out_off / out_len the raw bytes the
 * block consumed, crc its block CRC, stream 0, level the context's.  An empty input gives *count = 0, *npts = 0 and the 14-byte
 * stream.  The points are computed from what the encoder holds when a batch is packed (one wavefront a point), not by decoding.
 * BZH_E_ARG: an interval above 32767, a null count / npts, a null array with room claimed, and what bzh_encode_device refuses.
 * BZH_E_CAP: the output does not fit (as bzh_encode_device), or either array is too small: *count and *npts are then set and
 * everything else is unspecified, as for bzh_decode_index_sync.  Arrays sized by bzh_encode_index_bound never are too small.
 * The call runs on ONE lane (bzh_set_lanes does not apply), joins a streaming pass in flight and honours bzh_set_profiling
 * like every entry point.  After any error the context stays usable. */
BZH_API int bzh_encode_index_device(bzh_ctx *ctx, const void *d_in, size_t n, void *d_out, size_t cap, size_t *out_len,
                                    size_t *consumed, uint32_t interval, bzh_index_entry *idx, size_t max, size_t *count,
                                    bzh_sync_point *pts, size_t max_pts, size_t *npts);
/* Same, host buffers in and out (as bzh_encode). */
BZH_API int bzh_encode_index(bzh_ctx *ctx, const uint8_t *in, size_t n, uint8_t *out, size_t cap, size_t *out_len,
                             size_t *consumed, uint32_t interval, bzh_index_entry *idx, size_t max, size_t *count,
                             bzh_sync_point *pts, size_t max_pts, size_t *npts);
/* Pure host arithmetic, no context: array sizes that the call never exceeds for n input bytes at this level and interval.
 * With M = 100000 * level - 1: a block consumes at least M * 4 / 5 raw bytes, so *max_entries = n / (M * 4 / 5) + 2 (what
 * bzh_encode sizes its output by); a block has at most ceil((M + 1) / 50) = 2000 * level groups, so *max_pts = *max_entries *
 * ((2000 * level - 1) / interval), 0 for interval 0.  BZH_E_ARG: a level outside 1..9, an interval above 32767, a null pointer. */
BZH_API int bzh_encode_index_bound(int level, size_t n, uint32_t interval, size_t *max_entries, size_t *max_pts);

/* ---- streaming: encode() fed by a reader that yields arbitrary chunks (lib/rle.rs:30-92) ------- */

/* Starts a stream on the context.  Then call bzh_stream_feed any number of times; the bytes it
 * returns, concatenated, are exactly the stream bzh_encode produces for the concatenated input,
 * whatever the chunking (the reference's incremental InputStream + margin_call, without its T16
 * truncation bug).  Memory stays bounded: input is buffered only until the blocks it completes
 * are final (at most about one block's worth of raw bytes is carried between feeds). */
BZH_API int bzh_stream_begin(bzh_ctx *ctx);

/* Feeds n more input bytes; eof != 0 marks the end of the input (n may be 0) and completes the
 * stream.  Writes the stream bytes that became final to out; *out_len receives their count.
 * The bytes are copied to the GPU at once (`in` may be reused on return).  Once a full batch is
 * pending, a pass (split + encode + copy back) starts on an internal thread and the call returns;
 * its bytes are handed out by the next call that starts a pass, or by the eof call -- so the
 * caller's reading and copying of the next chunks overlaps with the GPU.
 * cap must be >= bzh_stream_bound(ctx, n) evaluated right before the call; BZH_E_CAP is returned
 * before anything is consumed (the call can be repeated with a larger buffer). */
BZH_API int bzh_stream_feed(bzh_ctx *ctx, const uint8_t *in, size_t n, int eof, uint8_t *out, size_t cap,
                            size_t *out_len);

/* Upper bound of the bytes the next bzh_stream_feed(…, n, …) call can return (depends on what is
 * pending and in flight, so ask before every call). */
BZH_API size_t bzh_stream_bound(const bzh_ctx *ctx, size_t n);

/* Pending input that triggers a GPU pass (default: one full batch, max_batch blocks of raw input, at most
 * 128 MiB; smaller = lower latency and less buffering, but more and smaller launches). */
BZH_API int bzh_stream_set_chunk(bzh_ctx *ctx, size_t bytes);

/* Input bytes encoded so far (after the eof feed: the total, encode()'s return value). */
BZH_API size_t bzh_stream_consumed(const bzh_ctx *ctx);

/* ---- the streaming encoder records its index: bzh_encode_index for inputs that are never resident as a whole ---------- */

/* bzh_stream_begin that also records the index of the stream being written: entries, and with interval in 1..32767 the sync
 * points of bzh_encode_index at that interval.  interval 0: entries only.  interval > 32767: BZH_E_ARG (the stream the context
 * had stays as it was).  The feeds, bzh_stream_bound, bzh_stream_set_chunk and bzh_stream_consumed are used as after
 * bzh_stream_begin, and the stream bytes are the same, whatever the chunking, in either Huffman mode.
 * Entries and points become FINAL when a feed collects the pass that encoded their blocks; after the eof feed everything is.
 * They are in STREAM coordinates, whatever the pass: bit_pos / end_bit count from bit 0 of the stream (the last block's end_bit
 * is the bit of the footer magic), out_off from byte 0 of the input, a point's entry is the block's number in the stream.  The
 * concatenation of everything taken equals, byte for byte, the arrays bzh_encode_index returns for the whole input at that
 * interval -- which are bzh_decode_index_sync's for the stream.  With an index a pass runs on ONE lane (bzh_set_lanes does not
 * apply), as bzh_encode_index does. */
BZH_API int bzh_stream_begin_index(bzh_ctx *ctx, uint32_t interval);

/* Entries and points that have become final and were not yet taken (both may be null).  A stream without index has none. */
BZH_API int bzh_stream_index_pending(const bzh_ctx *ctx, size_t *count, size_t *npts);

/* Moves them out, in order.  Either array too small: BZH_E_CAP, *count / *npts set, nothing removed.  A stream begun with
 * bzh_stream_begin (no index), or no stream at all: BZH_E_STATE.  idx may be null when max is 0, pts when max_pts is 0.
 * Allowed between feeds, after the eof feed and after a failed feed: a failed stream keeps what was pending until the next
 * begin.  Taking after every feed keeps the context's memory bounded: what waits is 40 bytes a block and 288 bytes per
 * `interval` x 50 symbols, some 2 % of the input at interval 256. */
BZH_API int bzh_stream_index_take(bzh_ctx *ctx, bzh_index_entry *idx, size_t max, size_t *count, bzh_sync_point *pts, size_t max_pts,
                                  size_t *npts);

/* ---- index files: pure host, no context, no GPU ----------------------------------------------------------------------- */

/* The file formats banzai_amd.BlockIndex.to_bytes() and SyncIndex.to_bytes() write, byte for byte.  All fields little-endian:
 *   interval 0 (block index):  "BZhIDX\r\n" | u32 version 1 | u32 reserved 0 | u64 entries | u64 consumed | the entries (40 bytes each)
 *   interval 1..32767:         "BZhSYN\r\n" | u32 version 1 | u32 interval | u64 bytes of the block index blob that follows | u64 points
 *                              | u32 CRC-32 | u32 reserved 0 | that block index blob | the points (288 bytes each)
 * `consumed` is the length of the indexed stream(s) in bytes (bzh_decode_index's *consumed, bzh_encode's *out_len).  The CRC-32
 * is zlib's, over the 40 header bytes with the CRC field zero and everything behind them.
 * bzh_index_blob_size: the bytes of the blob; 0 for an interval above 32767, points with interval 0, or a size beyond size_t. */
BZH_API size_t bzh_index_blob_size(size_t count, size_t npts, uint32_t interval);
/* Writes the blob to out[0..*out_len).  BZH_E_ARG: what bzh_index_blob_size answers with 0, a null out_len, a null array with a
 * count.  BZH_E_CAP: cap is below the size, which *out_len then holds.  The entries and points are written as given: whether
 * they are well formed is the decode calls' business. */
BZH_API int bzh_index_blob_write(const bzh_index_entry *idx, size_t count, const bzh_sync_point *pts, size_t npts, uint32_t interval,
                                 uint64_t consumed, uint8_t *out, size_t cap, size_t *out_len);
/* Reads a blob of either kind: a block index gives *interval = 0 and *npts = 0.  BZH_E_DATA: neither magic, another version, sizes
 * that do not add up to n exactly, a non-zero reserved field, an interval outside 1..32767 in a sync index, a CRC mismatch.
 * BZH_E_CAP: idx or pts is too small; *count and *npts are both set (as are *interval and *consumed), the arrays untouched: size
 * with one call (max = max_pts = 0, null arrays), fill with a second.  BZH_E_ARG: a null blob, count, npts, interval or
 * consumed, a null array with room claimed.  A block index blob carries no CRC: damage inside its entries is found by the
 * decode calls, which check every entry they use against the bytes. */
BZH_API int bzh_index_blob_read(const uint8_t *blob, size_t n, bzh_index_entry *idx, size_t max, size_t *count, bzh_sync_point *pts,
                                size_t max_pts, size_t *npts, uint32_t *interval, uint64_t *consumed);

/* ---- streaming decode: bzh_decode fed in chunks, bounded memory ------------------------------------------------ */

/* A stream decode holds a WINDOW of compressed bytes and a STAGING buffer of decoded bytes on the device, both its own (not
 * views of the decode workspace).  A PASS decodes what the window holds as far as it can be decided -- whole blocks, as many as
 * the staging buffer takes --, releases the input in front of the first item it could not decide and moves the rest to the
 * front of the window.  Only the bytes appended since the last pass are scanned for magics (from 6 bytes before them).
 * Memory: on the input side max(window target, the largest block the parser accepts: 4.1 MB) -- twice that while the tail is
 * moved, which goes from one buffer to another --, on the output side max(staging target, one block's decoded bytes: an RLE1
 * block of 900 kB can expand 51-fold), plus the batch workspace bzh_decode uses for as many candidates as the window holds.
 * The window grows, by what the call in hand still holds, only when it is full and its first item is still undecided; the
 * staging buffer grows only to a block that exceeds it.
 *
 * EQUIVALENCE.  For every split of an input into feeds and every sequence of cap values, the concatenated output is bzh_decode's
 * of the whole input, bzh_dstream_consumed its *consumed, the final status its status (BZH_E_ARG for a stream above the context's
 * level), and for an input with one defect bzh_last_error names the same kind, stream, block and absolute bit.  (With several
 * defects the one bzh_decode names depends on its batches; only the status is the same.)
 *
 * ERRORS.  The pass that finds a defect hands out nothing, the call returns the status, and the stream is closed: later feeds
 * are BZH_E_STATE until the next begin.  What earlier passes handed out is a prefix of the true output made of whole blocks whose
 * CRCs were verified; a STREAM CRC mismatch is found only at the stream's footer, after its blocks have gone out.  Unlike
 * bzh_decode a stream decode is therefore not all or nothing.  After an error bzh_dstream_consumed is the end of the last
 * footer the walk had passed up to the defect.
 *
 * Not here: a pass on an internal thread beside the caller's I/O (as bzh_stream_feed has), device-pointer variants, recovery
 * and index building on a stream, the multi-device handle. */
typedef struct {
    uint64_t passes, blocks, streams;
    uint64_t blocks_redone;   /* blocks whose entropy decode ran in more than one pass */
    uint64_t tail_moves, window_grows, staging_grows;
    uint64_t in_bytes, out_bytes;
    uint64_t window_peak, staging_peak;   /* bytes */
} bzh_dstream_stats;

/* Targets of the window and the staging buffer for the next bzh_dstream_begin.  0 = the default: 32 MiB of window, 128 MiB of
 * staging.  A non-zero value below 1024: BZH_E_ARG.  Small rooms mean many passes, and every pass costs at least one block's
 * serial entropy decode. */
BZH_API int bzh_dstream_set_room(bzh_ctx *ctx, size_t window_bytes, size_t staging_bytes);

/* Starts a stream decode on the context (abandoning one that is open).  Joins a streaming encode pass in flight. */
BZH_API int bzh_dstream_begin(bzh_ctx *ctx);

/* zlib-shaped: any n, any cap, no bound function.  In a loop the call hands staged bytes to out, returns when out is full,
 * copies input into the window while there is room (`in` may be reused on return), runs a pass when nothing is staged and the
 * window is full or eof has taken effect, and returns when all of `in` is used and nothing more can be handed out.
 * *in_used <= n: bytes of `in` taken; repeat the call with the rest when it is less.  eof != 0: `in` ends the input; it takes
 * effect once all n bytes of that call are used, so repeat the call with the rest and with eof again.  *out_len <= cap.
 * *done is set once the input is finished -- a footer followed by foreign bytes, or by the end of the input at eof -- and every
 * byte has been handed out; feeds after that succeed, use all of `in` and ignore it.
 * A call with n > 0 or pending output, and cap > 0, never returns BZH_OK having used no input, produced no output and not
 * set *done.  Passes are synchronous inside the call; between calls the context is idle and every other entry point may be
 * used on it (they do not disturb the stream).
 * BZH_E_ARG: a null ctx, in with n > 0, out with cap > 0, in_used, out_len or done; a stream above the context's level.
 * BZH_E_STATE: no begin, or the stream has ended in an error.  BZH_E_DATA as bzh_decode. */
BZH_API int bzh_dstream_feed(bzh_ctx *ctx, const uint8_t *in, size_t n, int eof, size_t *in_used, uint8_t *out, size_t cap,
                             size_t *out_len, int *done);

/* bzh_decode's *consumed, absolute: the first byte behind the padding of the last footer passed (0 for a null ctx). */
BZH_API size_t bzh_dstream_consumed(const bzh_ctx *ctx);

/* Counters of the stream since its begin (zeros before the first).  window_peak / staging_peak: the largest rooms held. */
BZH_API int bzh_dstream_get_stats(const bzh_ctx *ctx, bzh_dstream_stats *out);

/* Abandons the stream; always allowed (also with none open).  The buffers stay with the context for the next begin. */
BZH_API int bzh_dstream_end(bzh_ctx *ctx);

/* ---- block-sharded path (one rank per GPU) -------------------------- */

/* Split d_in[0..n) into blocks: the sequential part of the loop at lib/lib.rs:101-126, i.e.
 * every rle_one() cut (lib/rle.rs:102-253) and block CRC, without encoding anything.
 * The plan stays in the context and references d_in (caller keeps it alive). */
BZH_API int bzh_plan_device(bzh_ctx *ctx, const void *d_in, size_t n, size_t *nblocks);

/* The same in two steps, for a rank that continues another rank's split (banzai_amd/sharded.py): the loop of
 * lib/lib.rs:101-126 carries only `raw`, the stream CRC, `consumed` and the bit cursor from one block to the
 * next, so a rank needs nothing from its predecessor but the offset its first block starts at.
 * bzh_plan_tables_device builds the run tables of d_in[0..n) (no wait; they do not depend on where blocks start);
 * bzh_plan_split_device then cuts blocks from offset `start` of that buffer (a block start) until one starts at or
 * after `stop` (listed last: its offset is what the next rank needs; SIZE_MAX = to the end of the buffer), with or
 * without block CRCs.  Offsets in the resulting plan are relative to d_in. */
BZH_API int bzh_plan_tables_device(bzh_ctx *ctx, const void *d_in, size_t n);
BZH_API int bzh_plan_split_device(bzh_ctx *ctx, size_t start, size_t stop, int with_crc, size_t *nblocks);
BZH_API int bzh_plan_blocks(const bzh_ctx *ctx, bzh_block *out, size_t max_blocks);

/* The same split without the block CRCs (their `crc` fields read 0): for the sharded path, where every
 * rank splits the whole input but only encodes its own blocks.  bzh_encode_range_device computes the
 * CRCs of the range it encodes (they go into the block headers); bzh_plan_crc_range computes them on
 * request; afterwards bzh_plan_blocks reports them.  The rank that assembles the stream needs all of
 * them (bzh_assemble_device's block_crcs), so the ranks exchange them with their bit strings. */
BZH_API int bzh_plan_device_nocrc(bzh_ctx *ctx, const void *d_in, size_t n, size_t *nblocks);
BZH_API int bzh_plan_crc_range(bzh_ctx *ctx, size_t b0, size_t b1);

/* Per block of the plan: 1 if its cut is NOT final unless the planned input is the whole input -- the cut
 * lies in the input's last run, or the block reaches the end of the input (the streaming rule of
 * bzh_stream_feed).  A plan over a PREFIX of a longer input therefore yields the true blocks of the whole
 * input up to the first open one: ranks of the sharded path plan only as far as their own block range. */
BZH_API int bzh_plan_open(const bzh_ctx *ctx, uint8_t *out, size_t max_blocks);

/* Encode blocks [b0, b1) of the plan: per block the header (lib/lib.rs:24-36), symbol map
 * (:39-64) and Huffman payload (lib/huffman.rs:313-575), bit-concatenated from bit 0 of d_out
 * (MSB first, lib/out.rs), zero padded to a 4-byte multiple.  No stream header/footer. */
BZH_API int bzh_encode_range_device(bzh_ctx *ctx, size_t b0, size_t b1, void *d_out, size_t cap, uint64_t *nbits);

/* Stream assembly on one GPU: "BZh"+level (lib/lib.rs:18-22), the nseg bit strings
 * d_segs[k][0..seg_bits[k]) concatenated in order (funnel shift), footer + stream CRC folded
 * over block_crcs in block order (lib/lib.rs:66-70, :108), zero pad to a byte (lib/out.rs:22-28). */
BZH_API int bzh_assemble_device(bzh_ctx *ctx, const void *const *d_segs, const uint64_t *seg_bits, size_t nseg,
                        const uint32_t *block_crcs, size_t nblocks, void *d_out, size_t cap, size_t *out_len);

/* ---- several GPUs behind one handle: banzai::encode for a caller that holds a node (lib/lib.rs:84-88, the loop at
 * :101-126 sharded by start offset as above) -- one host thread and one context per listed device INSIDE the library,
 * the chain hand-off a host variable, the encoded bit strings copied to devices[0] (hipMemcpyPeer: xGMI) and
 * funnel-shifted into the stream there.  A device may be listed more than once (one context per entry: the whole
 * flow runs on a box with one GPU that way).  The handle is single-threaded like a context.  The launcher flow (one
 * process per GPU over torch.distributed, banzai_amd/sharded.py) remains for multi-process jobs. */
typedef struct bzh_multi bzh_multi;
BZH_API int bzh_create_multi(bzh_multi **out, const int *devices, int ndev, int level);
BZH_API void bzh_destroy_multi(bzh_multi *m);
BZH_API const char *bzh_multi_last_error(const bzh_multi *m);
BZH_API int bzh_multi_device_count(const bzh_multi *m);
/* Host buffers in and out: the complete .bz2 stream of in[0..n), bit-identical to bzh_encode's on one device. */
BZH_API int bzh_multi_encode(bzh_multi *m, const uint8_t *in, size_t n, uint8_t *out, size_t cap, size_t *out_len,
                             size_t *consumed);
/* The same in three steps (bench.py --single-process times the middle one: input resident in HBM when it starts,
 * the stream resident on devices[0] when it ends): every worker's byte range (+ look-ahead) to its device; tables,
 * chained split, encode, strings to devices[0], assembly; the stream back to host memory. */
BZH_API int bzh_multi_load(bzh_multi *m, const uint8_t *in, size_t n);
BZH_API int bzh_multi_run(bzh_multi *m, size_t *out_len);
BZH_API int bzh_multi_fetch(bzh_multi *m, uint8_t *out, size_t cap);
BZH_API const void *bzh_multi_output_device(const bzh_multi *m); /* the assembled stream on devices[0] (device pointer) */
/* Wall clocks of the last call per worker, 5 doubles each (ms): load, wait for the chain, tables + split, encode, copy. */
BZH_API int bzh_multi_times(const bzh_multi *m, double *out, size_t max_workers);
/* Test hook: the next runs give every worker a slab of `bytes` instead of the heuristic's (0 = the heuristic): a slab that is
 * too small is answered once with one of twice the size, a second overflow fails the call with BZH_E_CAP. */
BZH_API int bzh_multi_debug_slab(bzh_multi *m, size_t bytes);

/* ---- stage seams (host pointers; computed on the GPU; used by the parity tests) ------------ */

/* rle_one() applied repeatedly (lib/rle.rs:102-253): block table for in[0..n) and, if rle_out
 * is non-NULL, the RLE1 bytes of every block back to back (rle_cap bytes available). */
BZH_API int bzh_rle1_split(bzh_ctx *ctx, const uint8_t *in, size_t n, bzh_block *blocks, size_t max_blocks,
                   size_t *nblocks, uint8_t *rle_out, size_t rle_cap);

/* crc32::checksum (lib/crc32.rs:31-48). */
BZH_API int bzh_crc32(bzh_ctx *ctx, const uint8_t *in, size_t n, uint32_t *crc);

/* bwt::bwt (lib/bwt.rs:526-756) on nblk independent blocks: block k is
 * in[offs[k] .. offs[k]+lens[k]); bwt_out uses the same offsets; ptr[k]; has_byte[k*256..]. */
BZH_API int bzh_bwt_batch(bzh_ctx *ctx, const uint8_t *in, const uint64_t *offs, const uint32_t *lens, size_t nblk,
                  uint8_t *bwt_out, uint32_t *ptr, uint8_t *has_byte);
BZH_API int bzh_bwt(bzh_ctx *ctx, const uint8_t *in, size_t n, uint8_t *bwt_out, uint32_t *ptr, uint8_t *has_byte);

/* Verification tooling.  The reference has no decoder (README.md:9); its fuzz
 * target round-trips through libbz2 (fuzz/fuzz_targets/round_trip.rs:8-22).  bzh_unbwt_batch is the inverse of
 * bzh_bwt_batch computed on the GPU (one radix pass for the LF mapping, then pointer doubling): block k is
 * bwt[offs[k] .. offs[k]+lens[k]) with origin pointer ptr[k]; out receives the original bytes at the same offsets. */
BZH_API int bzh_unbwt_batch(bzh_ctx *ctx, const uint8_t *bwt, const uint64_t *offs, const uint32_t *lens,
                    const uint32_t *ptr, size_t nblk, uint8_t *out);

/* The same check without leaving the device, at any size: for blocks [b0, b1) of the current plan
 * (bzh_plan_device*), RLE1 bytes -> BWT -> inverse BWT, compared with the RLE1 bytes on the GPU.
 * *mismatches = number of differing bytes (0 when the transform is correct). */
BZH_API int bzh_bwt_roundtrip_device(bzh_ctx *ctx, size_t b0, size_t b1, uint64_t *mismatches);

/* mtf::mtf_and_rle (lib/mtf.rs:14-121): syms must hold n+1 entries, freqs 258. */
BZH_API int bzh_mtf(bzh_ctx *ctx, const uint8_t *bwt, size_t n, const uint8_t *has_byte, uint16_t *syms, size_t *m,
            uint32_t *freqs, uint32_t *num_syms);

/* Verification tooling: bzh_mtf on nblk columns in ONE launch, so that nblk decides the tile a wavefront walks (2,048
 * bytes below 64 blocks, 4,096 from 64 on) and chosen columns reach the tiles that whole streams reach only with whatever
 * their BWT gives.  Block k's column is bwt[offs[k] .. offs[k]+lens[k]), its present bytes has_byte[k*256..), its symbols
 * go to syms[offs[k]+k ..) (lens[k]+1 entries of room), m[k], freqs[k*258..), num_syms[k].  BZH_E_ARG for nblk == 0,
 * nblk > the context's max_batch, a length outside 1..block size, a null pointer. */
BZH_API int bzh_mtf_batch(bzh_ctx *ctx, const uint8_t *bwt, const uint64_t *offs, const uint32_t *lens, size_t nblk,
                  const uint8_t *has_byte, uint16_t *syms, uint32_t *m, uint32_t *freqs, uint32_t *num_syms);

/* huffman::encode (lib/huffman.rs:313-575) of one block as a standalone bit string from bit 0;
 * code_lengths (optional) receives num_tables x 258 final lengths, *num_tables the count. */
BZH_API int bzh_huffman(bzh_ctx *ctx, const uint16_t *syms, size_t m, uint32_t num_syms, const uint32_t *freqs,
                uint8_t *bits_out, size_t cap, uint64_t *nbits, uint8_t *code_lengths, uint32_t *num_tables);

/* The decoder's scan: the bit positions, ascending, of every occurrence of the block magic 0x314159265359 (kind 0) and of
 * the footer magic 0x177245385090 (kind 1) in in[0..n), at any bit alignment.  *count = occurrences; BZH_E_CAP if max is smaller. */
BZH_API int bzh_decode_scan(bzh_ctx *ctx, const uint8_t *in, size_t n, uint64_t *bitpos, uint8_t *kind, size_t max, size_t *count);

#ifdef __cplusplus
}
#endif
#endif /* BZHIP_H */
