// search_core.h -- THE TILE FRONT that search_tiles (search.hip) and grep_tiles (grep.hip) share, and what one thread of
// search_tiles does with its 16 bytes behind it.  The front: a thread's 16-byte load with the rule for the end of the text
// (bzf_load16), the pattern as a kernel argument (BzfPattern), the stores of a thread into the tile, its halo and the staged
// pattern (bzf_stage), and, behind the workgroup's barrier, the thread's hit mask: the filter on the pattern's first bytes and
// the verify of the rest (bzf_match16).  It lives here and nowhere else.  Plain C++ without a launch in it: the kernels compile it
// for the device, tests/decode_host/search_host.cpp and grep_host.cpp for the host, where this very text runs thread by thread
// and tile by tile over a model of the LDS, under ASan and UBSan, against a naive scan.
//
// THE LAYOUT.  A tile is BZF_TILE bytes of the text, thread t holds bytes [16 t, 16 t + 16) of it as four little-endian words and,
// for the filter, the word behind them.  Behind the tile lies a halo of plen - 1 bytes (the head of the next tile), so that a match
// that starts in the tile can be read to its end.  Positions are in the coordinates of the buffer the kernel is given:
//   [s_lo, s_hi)  the start positions that may be reported (s_hi <= n - plen + 1: a reported match ends inside the text),
//   [d_lo, n)     the bytes whose delimiters count (the carry in front of d_lo was counted by the window before).
// THE TEXT d[0, n) is 16-byte aligned, and what may be read of it ends with the aligned 4-byte word that holds byte n - 1.
#ifndef BZH_SEARCH_CORE_H
#define BZH_SEARCH_CORE_H
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define BZF_FN __host__ __device__ __forceinline__
#else
#define BZF_FN static inline
#endif

enum : uint32_t { BZF_THREADS = 256, BZF_ITEMS = 16, BZF_TILE = BZF_THREADS * BZF_ITEMS, BZF_MAX_PATTERN = 256 };

// the bytes of the word w that equal the byte `pat` repeats, bit j for byte j: the SWAR compare of count_bytes_blocks, its four
// flags gathered into four bits by one multiplication
BZF_FN uint32_t bzf_eq_mask4(uint32_t w, uint32_t pat)
{
    const uint32_t x = w ^ pat;
    const uint32_t t = ~((((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) | 0x7F7F7F7Fu); // 0x80 in every byte that is equal
    return (((t >> 7) * 0x00204081u) >> 21) & 15u;
}
// ... of a thread's 16 bytes w0 .. w3, bit k for byte k (the words are taken one by one: a thread's bytes stay in registers)
BZF_FN uint32_t bzf_eq_mask16(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t byte)
{
    const uint32_t pat = byte * 0x01010101u;
    return bzf_eq_mask4(w0, pat) | bzf_eq_mask4(w1, pat) << 4 | bzf_eq_mask4(w2, pat) << 8 | bzf_eq_mask4(w3, pat) << 12;
}

// the bits k of a thread whose position p0 + k lies in [lo, hi)
BZF_FN uint32_t bzf_range_mask16(uint64_t p0, uint64_t lo, uint64_t hi)
{
    const uint32_t a = lo > p0 ? (lo - p0 < 16 ? (uint32_t)(lo - p0) : 16u) : 0u;
    const uint32_t b = hi > p0 ? (hi - p0 < 16 ? (uint32_t)(hi - p0) : 16u) : 0u;
    return b > a ? ((1u << b) - 1u) & ~((1u << a) - 1u) : 0u;
}

// the delimiters of a thread in front of its byte k (dm: its delimiter bits, already cut to the bytes that count)
BZF_FN uint32_t bzf_delims_before(uint32_t dm, uint32_t k) { return (uint32_t)__builtin_popcount(dm & ((1u << k) - 1u)); }

// the pattern's first min(plen, 4) bytes as one word, and the mask of the bytes it has
BZF_FN uint32_t bzf_head_word(const uint8_t *pat, uint32_t plen)
{
    uint32_t v = 0;
    for (uint32_t j = 0; j < 4 && j < plen; j++) v |= (uint32_t)pat[j] << (8 * j);
    return v;
}
BZF_FN uint32_t bzf_head_mask(uint32_t plen) { return plen >= 4 ? 0xFFFFFFFFu : (1u << (8 * plen)) - 1u; }

// the filter for the four starts inside the word lo (hi: the word behind it): bit j when the bytes from byte j of lo on are the
// pattern's first ones
BZF_FN uint32_t bzf_filter4(uint32_t lo, uint32_t hi, uint32_t head, uint32_t mask)
{
    const uint64_t two = (uint64_t)hi << 32 | lo;
    return (uint32_t)((((uint32_t)two ^ head) & mask) == 0) | (uint32_t)((((uint32_t)(two >> 8) ^ head) & mask) == 0) << 1 |
           (uint32_t)((((uint32_t)(two >> 16) ^ head) & mask) == 0) << 2 | (uint32_t)((((uint32_t)(two >> 24) ^ head) & mask) == 0) << 3;
}
// the filter: the start positions k of a thread, of those in `valid`, whose first bytes are the pattern's.  w0 .. w3: the thread's
// 16 bytes, w4 the 4 behind them (bytes outside the text may hold anything: `valid` names no start whose match would reach them)
BZF_FN uint32_t bzf_filter16(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t w4, uint32_t valid, uint32_t head, uint32_t mask)
{
    return (bzf_filter4(w0, w1, head, mask) | bzf_filter4(w1, w2, head, mask) << 4 | bzf_filter4(w2, w3, head, mask) << 8 |
            bzf_filter4(w3, w4, head, mask) << 12) & valid;
}

// the verify: a start that passed the filter is a match when the bytes from the fifth on are the pattern's too.  text: the byte
// at the start position (the tile and its halo in the kernel); reads text[4 .. plen) and pat[4 .. plen)
BZF_FN bool bzf_verify(const uint8_t *text, const uint8_t *pat, uint32_t plen)
{
    for (uint32_t j = 4; j < plen; j++)
        if (text[j] != pat[j]) return false;
    return true;
}

// ---- the tile front ------------------------------------------------------------------------------------------------------------
struct alignas(16) BzfVec { // a thread's 16 bytes
    uint32_t x, y, z, w;
};

// A thread's 16 bytes at position p0 (a multiple of 16) of d[0, n).  Inside the text: one aligned 16-byte load.  At its end: the
// aligned 4-byte words that begin in front of n, zeros behind them -- no read goes past the word that holds byte n - 1.
BZF_FN BzfVec bzf_load16(const uint8_t *d, uint64_t n, uint64_t p0)
{
    if (p0 + 16 <= n) return *reinterpret_cast<const BzfVec *>(d + p0);
    BzfVec v;
    v.x = p0 < n ? *reinterpret_cast<const uint32_t *>(d + p0) : 0u;
    v.y = p0 + 4 < n ? *reinterpret_cast<const uint32_t *>(d + p0 + 4) : 0u;
    v.z = p0 + 8 < n ? *reinterpret_cast<const uint32_t *>(d + p0 + 8) : 0u;
    v.w = p0 + 12 < n ? *reinterpret_cast<const uint32_t *>(d + p0 + 12) : 0u;
    return v;
}

struct BzfPattern { // what is looked for, by value in the kernels' arguments
    uint32_t w[BZF_MAX_PATTERN / 4]; // the pattern, zeros behind it
    uint32_t plen;
    uint32_t head, hmask;            // the filter's word and mask
    uint32_t delim;
};
static inline BzfPattern bzf_pattern(const uint8_t *pat, uint32_t plen, uint32_t delim)
{
    BzfPattern p{};
    memcpy(p.w, pat, plen);
    p.plen = plen, p.head = bzf_head_word(pat, plen), p.hmask = bzf_head_mask(plen), p.delim = delim;
    return p;
}

// Thread tid of the tile at t0 stages its part: its 16 bytes into tile[BZF_TILE + BZF_MAX_PATTERN] (16-byte aligned), its share
// of the halo -- the head of the next tile, as far as a match that starts in this one can reach --, its word of the pattern into
// pat[BZF_MAX_PATTERN] (every lane reads the same byte of it).  Returns its 16 bytes.  A barrier follows.
BZF_FN BzfVec bzf_stage(const uint8_t *d, uint64_t n, uint64_t t0, uint32_t tid, const BzfPattern &p, uint8_t *tile, uint8_t *pat)
{
    if (tid < BZF_MAX_PATTERN / 4) reinterpret_cast<uint32_t *>(pat)[tid] = p.w[tid];
    const BzfVec own = bzf_load16(d, n, t0 + tid * BZF_ITEMS);
    *reinterpret_cast<BzfVec *>(tile + tid * BZF_ITEMS) = own;
    if (tid * BZF_ITEMS < p.plen - 1) *reinterpret_cast<BzfVec *>(tile + BZF_TILE + tid * BZF_ITEMS) = bzf_load16(d, n, t0 + BZF_TILE + tid * BZF_ITEMS);
    return own;
}

// Behind the barrier: the hit starts among the thread's 16 positions, of those in `valid`.  The word behind its bytes comes from
// the tile (thread 255: the halo's first word, or what lies there), the filter picks the candidates, and a pattern above four
// bytes is verified against the tile and its halo.
BZF_FN uint32_t bzf_match16(const BzfVec &own, uint32_t tid, const BzfPattern &p, const uint8_t *tile, const uint8_t *pat, uint32_t valid)
{
    const uint8_t *mine = tile + tid * BZF_ITEMS;
    uint32_t cand = bzf_filter16(own.x, own.y, own.z, own.w, *reinterpret_cast<const uint32_t *>(mine + BZF_ITEMS), valid, p.head, p.hmask);
    if (p.plen <= 4) return cand;
    uint32_t hm = 0;
    while (cand) {
        const uint32_t k = (uint32_t)__builtin_ctz(cand);
        cand &= cand - 1u;
        if (bzf_verify(mine + k, pat, p.plen)) hm |= 1u << k;
    }
    return hm;
}

#endif // BZH_SEARCH_CORE_H
