// crc_gf.h -- CRC-32/BZIP2 as arithmetic in GF(2)[x] mod P: the pieces the encoder's block CRCs (rle1.hip) and the decoder's
// CRC of an expansion that is never written (decode.hip) share.  A CRC register is a polynomial, bit 31 = x^31; the bytes of a
// message that lie in front of `k` more bytes weigh x^(8k), so pieces are folded on their own and shifted into place.
// tests/decode_host compiles the serial parts with g++.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define GF_FN __host__ __device__ __forceinline__
#else
#define GF_FN static inline
#endif

constexpr uint32_t CRC_POLY = 0x04C11DB7u;

struct CrcTables {
    uint32_t pow2[40];   // x^(2^k) mod P, k = 0..39 (bit exponents)
    uint32_t shift[256]; // x^(8*32*i) mod P: moves a 32-byte piece i pieces to the left
};

GF_FN uint32_t gf_mul(uint32_t a, uint32_t b) // a*b mod P, bit 31 = x^31
{
    uint32_t r = 0;
#if defined(__HIPCC__)
#pragma unroll 8
#endif
    for (int i = 31; i >= 0; i--) {
        r = (r << 1) ^ ((r >> 31) ? CRC_POLY : 0u);
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}

// x^e mod P for an exponent of the thread's own, e < 2^bits (bits <= 40): one multiplication per set bit.
GF_FN uint32_t gf_pow_x_serial(const uint32_t *pow2, uint64_t e, int bits)
{
    uint32_t f = 1u;
    for (int k = 0; k < bits; k++)
        if ((e >> k) & 1ull) f = gf_mul(f, pow2[k]);
    return f;
}

#if defined(__HIPCC__)
// x^e mod P for a wave-uniform exponent e (< 2^40): lanes take one bit each, product by butterfly.
__device__ __forceinline__ uint32_t gf_pow_x(const CrcTables &ct, uint64_t e, uint32_t lane)
{
    uint32_t f = 1u; // polynomial 1
    if (lane < 40 && ((e >> lane) & 1ull)) f = ct.pow2[lane];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) f = gf_mul(f, __shfl_xor(f, d, 64));
    return f;
}
#endif
