// decode_core.h -- the serial front of the bzip2 decoder: bit reader, block header parser, canonical decode tables, the
// symbol loop with the inverse MTF / RLE2, the footer, the state model of the inverse RLE1, and what one thread of the inverse
// RLE1 does with its 16 bytes: count, fold into a CRC, expand clipped to a window, count and locate a delimiter byte.
//
// One source, two builds.  decode.hip compiles it for gfx950, where ONE WAVEFRONT decodes one block: every lane runs the
// same serial code on the same values (so the bit window and the counters can live on the scalar side), and the lanes
// split what is parallel -- filling the look-up tables, shifting the MTF list, storing a run.  tests/decode_host compiles
// the very same text with g++ -fsanitize=address,undefined as a one-lane machine, which is where damaged streams are
// thrown at it by the thousand (sanitizers are a CPU affair).  Every read of the input is bounded by its length `n`, every
// index by the size of the table it goes into, every byte written by `block_max`: a damaged stream ends in a status.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIP_DEVICE_COMPILE__)
#define BZD_LANES 64u
#define BZD_LANE (threadIdx.x & 63u)
#define BZD_SYNC() __syncthreads() // (the decode kernel is one wavefront a workgroup)
#define BZD_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x))) // the lanes agree: keep the value on the scalar side
#define BZD_ANY(x) (__any((int)(x)) != 0)                                // true in some lane
#else
#define BZD_LANES 1u
#define BZD_LANE 0u
#define BZD_SYNC() ((void)0)
#define BZD_UNI(x) ((uint32_t)(x))
#define BZD_ANY(x) (x)
#endif
#if defined(__HIPCC__)
#define BZD_FN __host__ __device__ __forceinline__
#else
#define BZD_FN static inline
#endif

enum BzdKind : uint32_t { // what went wrong (bzh_last_error names it); 0 = the block decoded
    BZD_OK = 0,
    BZD_K_MAGIC = 1,      // no "BZh1".."BZh9" / no block or footer magic where the chain needs one
    BZD_K_TRUNC = 2,      // the input ends inside the stream
    BZD_K_FORMAT = 3,     // a field outside what the format allows
    BZD_K_BLOCK_CRC = 4,
    BZD_K_STREAM_CRC = 5,
    BZD_K_RANDOMISED = 6  // a randomised block (bzip2 0.9.0; no current encoder writes one)
};

constexpr uint32_t BZD_MAX_SEL = 32767, BZD_MAX_LEN = 20, BZD_GROUP = 50, BZD_LUT_BITS = 10;
constexpr uint64_t BZD_BLOCK_MAGIC = 0x314159265359ull, BZD_FOOTER_MAGIC = 0x177245385090ull;

struct BzdResult {
    uint32_t kind;    // BzdKind
    uint32_t crc;     // the stored CRC (block: of its bytes; footer: of the stream)
    uint64_t errpos;  // bit position where the parse gave up
    uint64_t end_bit; // first bit behind the block (footer: behind the padding)
    uint32_t nblock;  // bytes of the last column
    uint32_t origptr;
    uint32_t follow;  // footer only: 0 = the input ends behind it, 0x100 | level = "BZh<level>" follows, 2 = foreign bytes
    uint32_t pad;
};

struct BzdWork { // tables of the block being decoded (LDS on the GPU: 51 KB)
    uint16_t lut[6][1u << BZD_LUT_BITS]; // first 10 bits -> len << 9 | symbol (0: longer code, or none)
    int32_t limit[6][BZD_MAX_LEN + 2], base[6][BZD_MAX_LEN + 2];
    uint16_t perm[6][258];
    uint8_t len[6][258];
    uint32_t cnt[BZD_MAX_LEN + 2], start[BZD_MAX_LEN + 2];
    uint32_t minlen[6], maxlen[6];
    uint32_t bad;
    uint8_t sel[BZD_MAX_SEL + 1];
    uint8_t mtf[256];
};

// ---- bit reader: MSB first; `buf` holds the next `cnt` bits left-aligned, (pos + cnt) is a byte boundary.  Bits behind the
// input read as zero and bzd_over() turns true: callers check it wherever a decision has been taken on such bits.
struct BzdBits {
    const uint8_t *p;
    uint64_t n, pos, buf;
    uint32_t cnt;
};

BZD_FN uint32_t bzd_load32(const uint8_t *p, uint64_t n, uint64_t byte)
{
    uint32_t w = 0;
    if (byte + 4 <= n) {
        __builtin_memcpy(&w, p + byte, 4);
        return __builtin_bswap32(w);
    }
    for (uint32_t k = 0; k < 4; k++) w = (w << 8) | (byte + k < n ? (uint32_t)p[byte + k] : 0u);
    return w;
}

BZD_FN void bzd_seek(BzdBits &r, const uint8_t *p, uint64_t n, uint64_t pos)
{
    r.p = p;
    r.n = n;
    r.pos = pos;
    r.buf = 0;
    r.cnt = 0;
    const uint32_t sh = (uint32_t)(pos & 7u);
    if (sh) {
        const uint64_t byte = pos >> 3;
        const uint32_t b = byte < n ? BZD_UNI(p[byte]) : 0u;
        r.buf = (uint64_t)b << (56 + sh);
        r.cnt = 8 - sh;
    }
}

BZD_FN uint32_t bzd_peek(BzdBits &r, uint32_t k) // 1 <= k <= 32
{
    if (r.cnt < 32) {
        const uint32_t w = BZD_UNI(bzd_load32(r.p, r.n, (r.pos + r.cnt) >> 3));
        r.buf |= (uint64_t)w << (32 - r.cnt);
        r.cnt += 32;
    }
    return (uint32_t)(r.buf >> (64 - k));
}
BZD_FN void bzd_skip(BzdBits &r, uint32_t k) // after a peek of at least k bits
{
    r.buf <<= k;
    r.cnt -= k;
    r.pos += k;
}
BZD_FN uint32_t bzd_get(BzdBits &r, uint32_t k)
{
    const uint32_t v = bzd_peek(r, k);
    bzd_skip(r, k);
    return v;
}
BZD_FN bool bzd_over(const BzdBits &r) { return r.pos > r.n * 8; }

// ---- the front of a block, behind its magic: stored CRC, origPtr, symbol map, selectors, code lengths, and the canonical
// tables and look-up tables built from them.  `r` stands behind the 48 bits of the magic and is left at the first code.  True:
// `w` holds the tables, the selectors and the initial MTF list (the bytes in use, then zeros), h what the symbol loop needs;
// false: res.kind / res.errpos say what went wrong.  res.crc and res.origptr are set either way once they are read.
struct BzdHdr {
    uint32_t nin, nsel, ngroups;
};

BZD_FN bool bzd_parse_header(BzdWork &w, BzdBits &r, BzdResult &res, BzdHdr &h)
{
    const uint32_t lane = BZD_LANE;
    const bool l0 = lane == 0;
#define BZD_FAIL(k)         \
    do {                    \
        res.kind = (k);     \
        res.errpos = r.pos; \
        return false;       \
    } while (0)
    res.crc = bzd_get(r, 32);
    const uint32_t randomised = bzd_get(r, 1);
    const uint32_t origptr = bzd_get(r, 24);
    res.origptr = origptr;
    const uint32_t groups16 = bzd_get(r, 16);
    if (bzd_over(r)) BZD_FAIL(BZD_K_TRUNC);
    if (randomised) BZD_FAIL(BZD_K_RANDOMISED);
    // symbol map: the bytes in use, in order, straight into the MTF list
    uint32_t nin = 0;
    for (uint32_t g = 0; g < 16; g++) {
        if (!((groups16 >> (15 - g)) & 1u)) continue;
        const uint32_t bits = bzd_get(r, 16);
        for (uint32_t k = 0; k < 16; k++)
            if ((bits >> (15 - k)) & 1u) {
                if (l0) w.mtf[nin] = (uint8_t)(g * 16 + k);
                nin++;
            }
    }
    if (bzd_over(r)) BZD_FAIL(BZD_K_TRUNC);
    if (nin == 0) BZD_FAIL(BZD_K_FORMAT);
    for (uint32_t i = nin + lane; i < 256; i += BZD_LANES) w.mtf[i] = 0; // (never read by the loop: a sync point holds all 256)
    const uint32_t alpha = nin + 2;
    const uint32_t ngroups = bzd_get(r, 3), nsel = bzd_get(r, 15);
    if (bzd_over(r)) BZD_FAIL(BZD_K_TRUNC);
    if (ngroups < 2 || ngroups > 6 || nsel < 1) BZD_FAIL(BZD_K_FORMAT);
    { // selectors: unary-coded positions in a move-to-front list of the tables (six nibbles of one word)
        uint32_t order = 0x543210u;
        for (uint32_t i = 0; i < nsel; i++) {
            uint32_t j = 0;
            while (bzd_get(r, 1)) {
                if (++j >= ngroups) BZD_FAIL(BZD_K_FORMAT);
            }
            if (bzd_over(r)) BZD_FAIL(BZD_K_TRUNC);
            const uint32_t v = (order >> (4 * j)) & 15u, low = order & ((1u << (4 * j)) - 1u);
            order = (order & ~((1u << (4 * (j + 1))) - 1u)) | (low << 4) | v;
            if (l0) w.sel[i] = (uint8_t)v;
        }
    }
    for (uint32_t t = 0; t < ngroups; t++) { // delta-coded code lengths
        uint32_t cur = bzd_get(r, 5);
        for (uint32_t s = 0; s < alpha; s++) {
            for (;;) {
                if (cur < 1 || cur > BZD_MAX_LEN) BZD_FAIL(bzd_over(r) ? BZD_K_TRUNC : BZD_K_FORMAT);
                if (!bzd_get(r, 1)) break;
                cur = bzd_get(r, 1) ? cur - 1 : cur + 1;
                if (bzd_over(r)) BZD_FAIL(BZD_K_TRUNC);
            }
            if (l0) w.len[t][s] = (uint8_t)cur;
        }
        if (bzd_over(r)) BZD_FAIL(BZD_K_TRUNC);
    }
    if (l0) w.bad = 0;
    BZD_SYNC();
    // canonical codes: the symbols of one length are numbered in symbol order; an over-subscribed code is refused
    for (uint32_t t = 0; t < ngroups; t++) {
        if (l0) {
            for (uint32_t l = 0; l < BZD_MAX_LEN + 2; l++) w.cnt[l] = 0;
            uint32_t mn = 32, mx = 0;
            for (uint32_t s = 0; s < alpha; s++) {
                const uint32_t l = w.len[t][s];
                w.cnt[l]++;
                mn = l < mn ? l : mn;
                mx = l > mx ? l : mx;
            }
            int32_t code = 0, idx = 0;
            for (uint32_t l = mn; l <= mx; l++) {
                const int32_t c = (int32_t)w.cnt[l];
                w.base[t][l] = idx - code; // index into perm = code + base[l]
                w.start[l] = (uint32_t)idx;
                code += c;
                idx += c;
                w.limit[t][l] = code - 1; // largest code of this length
                if (code > (1 << l)) {
                    w.bad = 1;
                    break;
                }
                code <<= 1;
            }
            if (!w.bad)
                for (uint32_t s = 0; s < alpha; s++) {
                    const uint32_t l = w.len[t][s];
                    w.perm[t][w.start[l]++] = (uint16_t)s;
                }
            w.minlen[t] = mn;
            w.maxlen[t] = mx;
        }
        BZD_SYNC();
        if (BZD_UNI(w.bad)) BZD_FAIL(BZD_K_FORMAT);
        const uint32_t mn = BZD_UNI(w.minlen[t]), mx = BZD_UNI(w.maxlen[t]);
        for (uint32_t e = lane; e < (1u << BZD_LUT_BITS); e += BZD_LANES) { // the lanes fill the look-up table
            uint32_t entry = 0;
            for (uint32_t l = mn; l <= mx && l <= BZD_LUT_BITS; l++) {
                const int32_t code = (int32_t)(e >> (BZD_LUT_BITS - l));
                if (code <= w.limit[t][l]) {
                    const uint32_t idx = (uint32_t)(code + w.base[t][l]);
                    if (idx < alpha) entry = (l << 9) | w.perm[t][idx];
                    break;
                }
            }
            w.lut[t][e] = (uint16_t)entry;
        }
        BZD_SYNC();
    }
#undef BZD_FAIL
    h.nin = nin;
    h.nsel = nsel;
    h.ngroups = ngroups;
    return true;
}

// ---- symbols -> inverse RLE2 and MTF -> last column.  The loop's whole state between two symbols is the bit position, the
// selector index `gi`, the bytes written, the pending run and the MTF list: small enough to write down (a SYNC POINT) and to
// start from again.  W holds the tables and the MTF list (BzdWork, or a smaller set without selectors and lengths); `sel` the
// block's selectors, wherever they lie.
struct BzdSym {
    uint32_t gi;         // selector index of the next group
    uint32_t nblock;     // bytes written so far, counted from L (a pending run not included)
    uint32_t run;        // RUNA / RUNB run accumulated so far, 0 = none
    uint32_t run_weight; // weight of the next run digit, 1 = none pending
    uint32_t eob;        // the end-of-block symbol was met
};

struct BzdNoRec { // the recorder that records nothing
    static constexpr bool ON = false;
    uint32_t interval = 1;
    BZD_FN void point(uint64_t, uint32_t, uint32_t, uint32_t, uint32_t, const uint8_t *) {}
};

// Runs from the state in `s` (r at its bit position, at a group boundary) to the end of the block, or, with gi_stop != 0, to
// the boundary in front of group gi_stop.  Not more than out_max bytes are written to L.  Returns a BzdKind (r.pos is where);
// `s` is the state it stopped in.  Where a group begins whose index is a multiple of rec.interval, the recorder is handed
// the state first (recording builds only).
template <class W, class Rec>
BZD_FN uint32_t bzd_symbols(W &w, const uint8_t *sel, BzdBits &r, uint32_t nin, uint32_t nsel, uint32_t gi_stop, uint32_t out_max, uint8_t *L,
                            BzdSym &s, Rec &rec)
{
    const uint32_t lane = BZD_LANE;
    const bool l0 = lane == 0;
    const uint32_t alpha = nin + 2, eob = alpha - 1;
    uint32_t nblock = s.nblock, run = s.run, run_weight = s.run_weight, gi = s.gi, group_left = 0, t = 0, mn = 0, mx = 0;
#define BZD_FAIL(k)                  \
    do {                             \
        s.gi = gi;                   \
        s.nblock = nblock;           \
        s.run = run;                 \
        s.run_weight = run_weight;   \
        return (k);                  \
    } while (0)
    s.eob = 0;
    for (;;) {
        if (group_left == 0) {
            if (gi_stop && gi == gi_stop) BZD_FAIL(BZD_OK); // (not a failure: the segment ends here)
            if (gi >= nsel) BZD_FAIL(BZD_K_FORMAT);
            if (Rec::ON && gi > 0 && gi % rec.interval == 0) rec.point(r.pos, gi, nblock, run, run_weight, w.mtf);
            t = BZD_UNI(sel[gi]);
            gi++;
            group_left = BZD_GROUP;
            mn = BZD_UNI(w.minlen[t]);
            mx = BZD_UNI(w.maxlen[t]);
        }
        group_left--;
        const uint32_t bits = bzd_peek(r, BZD_MAX_LEN);
        const uint32_t e = BZD_UNI(w.lut[t][bits >> (BZD_MAX_LEN - BZD_LUT_BITS)]);
        uint32_t l, sym;
        if (e) {
            l = e >> 9;
            sym = e & 511u;
        } else { // a code longer than the table's index, or none at all
            l = mn;
            while (l <= mx && (int32_t)(bits >> (BZD_MAX_LEN - l)) > (int32_t)BZD_UNI(w.limit[t][l])) l++;
            if (l > mx) BZD_FAIL(r.pos + mx > r.n * 8 ? BZD_K_TRUNC : BZD_K_FORMAT);
            const uint32_t idx = (bits >> (BZD_MAX_LEN - l)) + BZD_UNI(w.base[t][l]);
            if (idx >= alpha) BZD_FAIL(BZD_K_FORMAT);
            sym = BZD_UNI(w.perm[t][idx]);
        }
        bzd_skip(r, l);
        if (bzd_over(r)) BZD_FAIL(BZD_K_TRUNC);
        if (sym <= 1) { // RUNA / RUNB: bijective base-2 digits of a run of the front byte
            if (run_weight > (1u << 21)) BZD_FAIL(BZD_K_FORMAT);
            run += run_weight << sym;
            run_weight <<= 1;
            continue;
        }
        if (run) {
            const uint32_t b = BZD_UNI(w.mtf[0]);
            if (run > out_max - nblock) BZD_FAIL(BZD_K_FORMAT);
            for (uint32_t i = lane; i < run; i += BZD_LANES) L[nblock + i] = (uint8_t)b; // whole-wave stores
            nblock += run;
            run = 0;
            run_weight = 1;
        }
        if (sym == eob) break;
        const uint32_t p = sym - 1; // MTF position, >= 1
        if (p >= nin) BZD_FAIL(BZD_K_FORMAT);
        const uint32_t v = BZD_UNI(w.mtf[p]);
        // mtf[1 .. p] = mtf[0 .. p-1], from the top down, 64 entries at a time: a slice reads before it writes, and what it
        // reads lies below what the slices before it wrote
        for (uint32_t j0 = 0; j0 < p; j0 += BZD_LANES) {
            const uint32_t j = j0 + lane;
            const bool act = j < p;
            const uint8_t tv = act ? w.mtf[p - j - 1] : (uint8_t)0;
            BZD_SYNC();
            if (act) w.mtf[p - j] = tv;
            BZD_SYNC();
        }
        if (l0) w.mtf[0] = (uint8_t)v;
        BZD_SYNC();
        if (nblock >= out_max) BZD_FAIL(BZD_K_FORMAT);
        if (l0) L[nblock] = (uint8_t)v;
        nblock++;
    }
    s.eob = 1;
    BZD_FAIL(BZD_OK);
#undef BZD_FAIL
}

// ---- one block: `pos` = bit position of its magic.  Leaves the last column in L[0 .. nblock), nblock <= block_max.
template <class Rec>
BZD_FN void bzd_decode_block_rec(BzdWork &w, const uint8_t *in, uint64_t n, uint64_t pos, uint32_t block_max, uint8_t *L, BzdResult &res,
                                 Rec &rec)
{
    BzdBits r;
    bzd_seek(r, in, n, pos + 48);
    res.kind = BZD_OK;
    res.errpos = 0;
    res.end_bit = 0;
    res.nblock = 0;
    res.follow = 0;
    res.pad = 0;
    BzdHdr h;
    if (!bzd_parse_header(w, r, res, h)) return;
    BzdSym s = {0, 0, 0, 1, 0};
    const uint32_t kind = bzd_symbols(w, w.sel, r, h.nin, h.nsel, 0u, block_max, L, s, rec);
    if (kind != BZD_OK) {
        res.kind = kind;
        res.errpos = r.pos;
        return;
    }
    res.nblock = s.nblock;
    if (s.nblock == 0 || res.origptr >= s.nblock) {
        res.kind = BZD_K_FORMAT;
        res.errpos = r.pos;
        return;
    }
    res.end_bit = r.pos;
}

BZD_FN void bzd_decode_block(BzdWork &w, const uint8_t *in, uint64_t n, uint64_t pos, uint32_t block_max, uint8_t *L, BzdResult &res)
{
    BzdNoRec rec;
    bzd_decode_block_rec(w, in, n, pos, block_max, L, res, rec);
}

// ---- a SEGMENT of a block: from one sync point (or from the header's state, group 0) to the next (or to the end of the block).
// The state of a point, as the symbol loop hands it to a recorder; bit_pos in the coordinates of `in`.
struct BzdSyncState {
    uint64_t bit_pos;
    uint32_t group, out_pos, run, run_weight;
    const uint8_t *mtf; // 256 bytes
};

enum BzdSegMiss : uint32_t { // why a segment does not fit its points (0: it does)
    BZD_SEG_OK = 0,
    BZD_SEG_START = 1, // the point it starts from cannot be a state of this block
    BZD_SEG_EOB = 2,   // the block ends in front of the next point
    BZD_SEG_ARRIVE = 3 // it arrives at the next point's group in another state than the point holds
};

struct BzdSegResult {
    uint32_t kind; // BzdKind of the symbol loop
    uint32_t miss; // BzdSegMiss
    uint64_t errpos;
    uint64_t end_bit; // last segment: first bit behind the block
    uint32_t nblock;  // last segment: bytes of the whole last column
    uint32_t pad;
};

// Decodes from `from` to `to` (has_to false: to the end of the block, `to` is not looked at).  `out` is where byte from.out_pos of the last column goes: at most
// to.out_pos - from.out_pos bytes are written there (last segment: block_max - from.out_pos).  Points are untrusted: whatever
// they hold, every index stays inside its table and every store inside that room, and a segment that does not arrive exactly
// at `to` says so.  w: tables of the block's header; its MTF list is loaded from the point here.
template <class W>
BZD_FN void bzd_decode_segment(W &w, const uint8_t *sel, const uint8_t *in, uint64_t n, uint32_t nin, uint32_t nsel, uint32_t origptr,
                               const BzdSyncState &from, bool has_to, const BzdSyncState &to, uint32_t block_max, uint8_t *out,
                               BzdSegResult &res)
{
    const uint32_t lane = BZD_LANE;
    res.kind = BZD_OK;
    res.miss = BZD_SEG_OK;
    res.errpos = from.bit_pos;
    res.end_bit = 0;
    res.nblock = 0;
    res.pad = 0;
    const uint32_t out_end = has_to ? to.out_pos : block_max, gi_stop = has_to ? to.group : 0u;
    if (from.out_pos > out_end || out_end > block_max || from.group >= nsel || (has_to && to.group <= from.group) || from.bit_pos > n * 8 ||
        from.run_weight == 0 || from.run_weight > (1u << 22)) {
        res.miss = BZD_SEG_START;
        return;
    }
    for (uint32_t i = lane; i < 256; i += BZD_LANES) w.mtf[i] = from.mtf[i];
    BZD_SYNC();
    BzdBits r;
    bzd_seek(r, in, n, from.bit_pos);
    BzdSym s = {from.group, 0, from.run, from.run_weight, 0};
    BzdNoRec rec;
    const uint32_t kind = bzd_symbols(w, sel, r, nin, nsel, gi_stop, out_end - from.out_pos, out, s, rec);
    res.errpos = r.pos;
    if (kind != BZD_OK) {
        res.kind = kind;
        return;
    }
    if (!has_to) {
        res.nblock = from.out_pos + s.nblock;
        res.end_bit = r.pos;
        if (res.nblock == 0 || origptr >= res.nblock) res.kind = BZD_K_FORMAT;
        return;
    }
    if (s.eob) {
        res.miss = BZD_SEG_EOB;
        return;
    }
    bool differs = false;
    for (uint32_t i = lane; i < 256; i += BZD_LANES) differs |= w.mtf[i] != to.mtf[i];
    if (BZD_ANY(differs) || r.pos != to.bit_pos || from.out_pos + s.nblock != to.out_pos || s.run != to.run || s.run_weight != to.run_weight)
        res.miss = BZD_SEG_ARRIVE;
}

// ---- sync points are untrusted input (they may come from a file): what makes point i of pts[0 .. npts) ill formed against the
// index idx[0 .. count), whatever the bytes hold (null: nothing).  E: bzh_index_entry, P: bzh_sync_point (include/bzhip.h).
template <class E, class P>
static inline const char *bzd_sync_point_check(const E *idx, size_t count, const P *pts, size_t i)
{
    const P &p = pts[i];
    if (p.reserved != 0) return "reserved is not 0";
    if (p.group == 0 || p.group >= BZD_MAX_SEL) return "group outside 1..32766";
    if (p.entry >= count) return "entry outside the index";
    const E &e = idx[p.entry];
    const bool same = i > 0 && pts[i - 1].entry == p.entry;
    if (i > 0 && (pts[i - 1].entry > p.entry || (same && pts[i - 1].group >= p.group))) return "(entry, group) does not ascend";
    if (p.bit_pos <= e.bit_pos || p.bit_pos >= e.end_bit) return "bit_pos is not inside its entry";
    if (same && p.bit_pos <= pts[i - 1].bit_pos) return "bit_pos does not ascend";
    if (same && p.out_pos < pts[i - 1].out_pos) return "out_pos descends";
    if (e.level < 1 || e.level > 9 || p.out_pos > 100000u * e.level) return "out_pos beyond the level's block size";
    const uint32_t rw = p.run_weight;
    if (rw == 0 || (rw & (rw - 1)) != 0 || rw > (1u << 22)) return "run_weight is no power of two up to 2^22";
    if (p.run + 1 < rw || p.run + 1 > 2 * rw - 1) return "run and run_weight do not belong together";
    return nullptr;
}

// ---- the footer at bit `pos` (its magic): stream CRC, padding to a byte, and what follows
BZD_FN void bzd_parse_footer(const uint8_t *in, uint64_t n, uint64_t pos, BzdResult &res)
{
    BzdBits r;
    bzd_seek(r, in, n, pos + 48);
    res.kind = BZD_OK;
    res.errpos = 0;
    res.nblock = 0;
    res.origptr = 0;
    res.follow = 0;
    res.pad = 0;
    res.crc = bzd_get(r, 32);
    const uint64_t end = (r.pos + 7) >> 3;
    res.end_bit = end * 8;
    if (bzd_over(r)) {
        res.kind = BZD_K_TRUNC;
        res.errpos = r.n * 8;
        return;
    }
    if (end == n) return;
    res.follow = 2;
    if (end + 4 <= n) {
        const uint32_t h = BZD_UNI(bzd_load32(in, n, end));
        const uint32_t lv = h & 255u;
        if ((h >> 8) == 0x425A68u && lv >= '1' && lv <= '9') res.follow = 0x100u | (lv - '0');
    }
}

// ---- inverse RLE1 as a state machine: four equal bytes, then a count byte (libbz2's rule; the state resets behind a count
// byte and at the block start).  State = equal bytes seen so far, 0..4; the byte met in state 4 is a count byte.  A byte's
// transition depends only on whether it equals the byte before it, so a stretch of bytes is a map {0..4} -> {0..4} (three
// bits a state) and maps compose: which bytes are count bytes comes out of a scan, not out of a walk.
constexpr uint32_t BZD_RL_EQ = 1u | 2u << 3 | 3u << 6 | 4u << 9 | 0u << 12; // the byte equals its predecessor
constexpr uint32_t BZD_RL_NE = 1u | 1u << 3 | 1u << 6 | 1u << 9 | 0u << 12; // it does not (or the block starts)
constexpr uint32_t BZD_RL_ID = 0u | 1u << 3 | 2u << 6 | 3u << 9 | 4u << 12;
BZD_FN uint32_t bzd_rl_apply(uint32_t m, uint32_t s) { return (m >> (3 * s)) & 7u; }
BZD_FN uint32_t bzd_rl_compose(uint32_t first, uint32_t then)
{
    uint32_t r = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t s = 0; s < 5; s++) r |= bzd_rl_apply(then, bzd_rl_apply(first, s)) << (3 * s);
    return r;
}
BZD_FN uint32_t bzd_rl_step(uint32_t s, bool eq) { return s == 4 ? 0u : (eq && s >= 1 ? s + 1 : 1u); }

// ---- one thread's stretch of a block behind the inverse BWT: cnt <= 16 bytes, byte k in bits 8*(k&3) of w[k>>2]; `prev` the
// byte before them (256: none), `s` the state they are entered in.  In state 4 a byte is a count: it stands for that many
// copies of the byte before it (0..255); any other byte stands for itself.
constexpr uint32_t BZD_UR_ITEMS = 16;
BZD_FN uint32_t bzd_ur_at(const uint32_t *w, uint32_t k) { return (w[k >> 2] >> (8 * (k & 3))) & 255u; }

// The stretch as a map of states: where each of the five states it could be entered in has got to behind its last byte.
BZD_FN uint32_t bzd_ur_map(const uint32_t *w, uint32_t cnt, uint32_t prev)
{
    uint32_t st[5] = {0, 1, 2, 3, 4};
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t k = 0; k < BZD_UR_ITEMS; k++) {
        if (k < cnt) {
            const uint32_t c = bzd_ur_at(w, k);
            const bool eq = c == prev;
#if defined(__HIPCC__)
#pragma unroll
#endif
            for (int q = 0; q < 5; q++) st[q] = bzd_rl_step(st[q], eq);
            prev = c;
        }
    }
    return st[0] | st[1] << 3 | st[2] << 6 | st[3] << 9 | st[4] << 12;
}

// How many bytes the stretch expands to; *s_end = the state behind its last byte.
BZD_FN uint32_t bzd_ur_size(const uint32_t *w, uint32_t cnt, uint32_t prev, uint32_t s, uint32_t *s_end)
{
    uint32_t o = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t k = 0; k < BZD_UR_ITEMS; k++) {
        if (k < cnt) {
            const uint32_t c = bzd_ur_at(w, k);
            o += s == 4 ? c : 1u;
            s = bzd_rl_step(s, c == prev);
            prev = c;
        }
    }
    *s_end = s;
    return o;
}

// The CRC register (CRC-32/BZIP2 without its init and final XOR: the polynomial of the bytes alone) over what the stretch
// expands to, *outn = how many bytes that is.  tab[v] = v * x^32 mod P.  Nothing is written: at most 16 * 255 table steps.
BZD_FN uint32_t bzd_ur_fold(const uint32_t *tab, const uint32_t *w, uint32_t cnt, uint32_t prev, uint32_t s, uint32_t *outn)
{
    uint32_t crc = 0, o = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t k = 0; k < BZD_UR_ITEMS; k++) {
        if (k < cnt) {
            const uint32_t c = bzd_ur_at(w, k);
            if (s == 4) {
                for (uint32_t q = 0; q < c; q++) crc = (crc << 8) ^ tab[(crc >> 24) ^ prev];
                o += c;
            } else {
                crc = (crc << 8) ^ tab[(crc >> 24) ^ c];
                o++;
            }
            s = bzd_rl_step(s, c == prev);
            prev = c;
        }
    }
    *outn = o;
    return crc;
}

// [*a, *b) = the part of [o, o + len) inside the window [lo, hi); empty (*a == *b) when they do not meet
BZD_FN void bzd_clip(uint32_t o, uint32_t len, uint32_t lo, uint32_t hi, uint32_t *a, uint32_t *b)
{
    const uint32_t e = o + len;
    *a = o > lo ? o : lo;
    *b = e < hi ? e : hi;
    if (*b < *a) *b = *a;
}

// What a tile of `len` output bytes at `toff` of its block owes a piece: bytes [lo, hi) of the block's own output, wanted at
// `base` of an output of out_total bytes.  [*a, *b) = the piece inside the tile, in the tile's own bytes; *dst = where byte *a
// goes.  False: the two do not meet -- or the bytes would not lie inside the output, which no table may make a kernel leave.
BZD_FN bool bzd_piece_cut(uint32_t toff, uint32_t len, uint32_t lo, uint32_t hi, uint64_t base, uint64_t out_total, uint32_t *a, uint32_t *b,
                          uint64_t *dst)
{
    bzd_clip(toff, len, lo, hi, a, b);
    if (*a >= *b) return false;
    *dst = base + (*a - lo);
    if (*dst < base || *dst >= out_total || *b - *a > out_total - *dst) return false;
    *a -= toff;
    *b -= toff;
    return true;
}

// The expansion of the stretch, which begins at output position o: put(position, byte) for every position inside [lo, hi) and
// for no other.  A run that lies outside the window costs nothing.
template <class Put>
BZD_FN void bzd_ur_emit(const uint32_t *w, uint32_t cnt, uint32_t prev, uint32_t s, uint32_t o, uint32_t lo, uint32_t hi, Put put)
{
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t k = 0; k < BZD_UR_ITEMS; k++) {
        if (k < cnt) {
            const uint32_t c = bzd_ur_at(w, k);
            const uint32_t len = s == 4 ? c : 1u, byte = s == 4 ? prev : c;
            uint32_t a, b;
            bzd_clip(o, len, lo, hi, &a, &b);
            for (uint32_t q = a; q < b; q++) put(q, (uint8_t)byte);
            o += len;
            s = bzd_rl_step(s, c == prev);
            prev = c;
        }
    }
}

// ---- records: the delimiter bytes of the expansion, counted and located with nothing written (unrle_count / unrle_select).
// A count byte is never a literal: met in state 4, the byte c stands for c copies of the byte before it and for nothing else, so
// "aaaa\x0a" is fourteen 'a' and no newline, and "\n\n\n\n\x03" is seven newlines.
// How many bytes equal to `delim` the stretch expands to; *outn = how many bytes it expands to, *last = the last byte of the
// expansion of everything up to the stretch's end (a count byte of 0 writes nothing, and the byte in front of it is its run's),
// left as it is by an empty stretch.
BZD_FN uint32_t bzd_ur_count(const uint32_t *w, uint32_t cnt, uint32_t prev, uint32_t s, uint32_t delim, uint32_t *outn, uint32_t *last)
{
    uint32_t d = 0, o = 0;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t k = 0; k < BZD_UR_ITEMS; k++) {
        if (k < cnt) {
            const uint32_t c = bzd_ur_at(w, k);
            const uint32_t len = s == 4 ? c : 1u, byte = s == 4 ? prev : c;
            d += byte == delim ? len : 0u;
            o += len;
            *last = byte;
            s = bzd_rl_step(s, c == prev);
            prev = c;
        }
    }
    *outn = o;
    return d;
}

// Where the k-th (1-based) delimiter of the stretch lies, counted in bytes of the stretch's own expansion; inside a run, the exact
// byte of the run.  0xFFFFFFFF: the stretch holds fewer than k, or k is 0.
BZD_FN uint32_t bzd_ur_select(const uint32_t *w, uint32_t cnt, uint32_t prev, uint32_t s, uint32_t delim, uint32_t k)
{
    uint32_t o = 0, at = 0xFFFFFFFFu;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t i = 0; i < BZD_UR_ITEMS; i++) {
        if (i < cnt) {
            const uint32_t c = bzd_ur_at(w, i);
            const uint32_t len = s == 4 ? c : 1u, byte = s == 4 ? prev : c;
            const uint32_t here = byte == delim ? len : 0u;
            if (k >= 1 && k <= here && at == 0xFFFFFFFFu) at = o + k - 1;
            k = k > here ? k - here : 0u; // (0 once found or once impossible: nothing behind it matches)
            o += len;
            s = bzd_rl_step(s, c == prev);
            prev = c;
        }
    }
    return at;
}
