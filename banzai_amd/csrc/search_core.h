// search_core.h -- what ONE THREAD of search_tiles (search.hip) does with its 16 bytes: which of them are the delimiter, which of
// its 16 start positions pass the filter on the pattern's first bytes, and whether the rest of the pattern follows.  Plain C++
// without a launch in it: the kernel compiles it for the device, tests/decode_host/search_host.cpp for the host, where it runs
// thread by thread and tile by tile in the kernel's layout against a naive scan.
//
// THE LAYOUT.  A tile is BZF_TILE bytes of the text, thread t holds bytes [16 t, 16 t + 16) of it as four little-endian words and,
// for the filter, the word behind them.  Behind the tile lies a halo of plen - 1 bytes (the head of the next tile), so that a match
// that starts in the tile can be read to its end.  Positions are in the coordinates of the buffer the kernel is given:
//   [s_lo, s_hi)  the start positions that may be reported (s_hi <= n - plen + 1: a reported match ends inside the text),
//   [d_lo, n)     the bytes whose delimiters count (the carry in front of d_lo was counted by the window before).
#ifndef BZH_SEARCH_CORE_H
#define BZH_SEARCH_CORE_H
#include <stddef.h>
#include <stdint.h>

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

#endif // BZH_SEARCH_CORE_H
