// recover_gather.h -- what ONE destination word of bzh_recover_stream's body holds: the bits of the kept blocks, each of which
// starts at a source bit of its own, laid end to end from bit 32 of the output.  One source, two builds, as decode_core.h:
// recover.hip compiles it for gfx950, a thread a destination word; tests/decode_host/gather_host.cpp compiles the same text with
// g++ -fsanitize=address,undefined and holds it against a bit-by-bit copy.  Every read of the source goes through bzd_load32 and
// is bounded by its length `n`, whatever a descriptor holds; the caller bounds the destination words.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "decode_core.h" // BZD_FN, bzd_load32

struct BzrDesc {      // one kept block
    uint64_t src_bit; // of its magic in the input
    uint64_t dst_bit; // where it goes: 32 + the bits of the blocks before it (ascending)
    uint64_t nbits;
};

// The first descriptor that ends behind destination bit `bit` (K: none does).  The ends ascend: a binary search.
BZD_FN uint32_t bzr_find(const BzrDesc *d, uint32_t K, uint64_t bit)
{
    uint32_t lo = 0, hi = K;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (d[mid].dst_bit + d[mid].nbits <= bit)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// Destination word `word` (bits [32 word, 32 word + 32), MSB first, as a big-endian value): the bits every descriptor that
// covers it puts there, zero elsewhere.  k: a descriptor at or in front of the first that covers the word (bzr_find of this word's
// first bit, or of an earlier word's: the walk from there is linear).  A word can straddle a block edge, so it loops over the
// covering descriptors; each piece is a two-word funnel of the source, masked to its length.
BZD_FN uint32_t bzr_gather_word(const BzrDesc *d, uint32_t K, uint32_t k, uint64_t word, const uint8_t *src, uint64_t n)
{
    const uint64_t lo = word * 32, hi = lo + 32;
    while (k < K && d[k].dst_bit + d[k].nbits <= lo) k++;
    uint32_t v = 0;
    for (; k < K && d[k].dst_bit < hi; k++) {
        const uint64_t d0 = d[k].dst_bit, d1 = d0 + d[k].nbits;
        const uint64_t a = d0 > lo ? d0 : lo, b = d1 < hi ? d1 : hi; // the piece, in destination bits
        if (b <= a) continue;                                        // (a descriptor of no bits)
        const uint32_t cnt = (uint32_t)(b - a);                     // 1..32
        const uint64_t s = d[k].src_bit + (a - d0);
        const uint32_t sh = (uint32_t)(s & 7u);
        const uint32_t w0 = bzd_load32(src, n, s >> 3), w1 = sh ? bzd_load32(src, n, (s >> 3) + 4) : 0u;
        uint32_t x = sh ? (w0 << sh) | (w1 >> (32 - sh)) : w0;      // the 32 bits from source bit s on
        if (cnt < 32) x &= ~(0xFFFFFFFFu >> cnt);                   // the piece's own bits only
        v |= x >> (uint32_t)(a - lo);
    }
    return v;
}
