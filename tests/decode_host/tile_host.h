// tile_host.h -- what search_host.cpp and grep_host.cpp share: a text allocated as the kernels' contract states, and the model of a
// workgroup's LDS over which the tile front of banzai_amd/csrc/search_core.h -- bzf_stage and bzf_match16, the kernels' own text --
// runs thread by thread.  Nothing here loads, stages, filters or verifies on its own.
#ifndef BZH_TILE_HOST_H
#define BZH_TILE_HOST_H
#include <stdlib.h>
#include <string.h>

#include "../../banzai_amd/csrc/search_core.h"

// A text d[0, n) as search_tiles and grep_tiles are given it: 16-byte aligned, and it ends with the aligned 4-byte word that holds
// byte n - 1, so a read behind that word is a sanitizer report.  The bytes of that word behind n hold `slack`: a value that is
// neither the pattern's nor the delimiter's.
struct Text {
    uint8_t *p = nullptr;
    explicit Text(uint64_t n, uint8_t slack = 0xEE)
    {
        const size_t size = (size_t)((n + 3) & ~(uint64_t)3);
        if (posix_memalign((void **)&p, 16, size ? size : 1)) abort(); // (n == 0: one byte that nobody may touch)
        memset(p, slack, size ? size : 1);
    }
    Text(const uint8_t *src, uint64_t n, uint8_t slack = 0xEE) : Text(n, slack)
    {
        if (n) memcpy(p, src, (size_t)n);
    }
    ~Text() { free(p); }
};

// One workgroup: the two LDS arrays of the kernels at their exact sizes, and every thread's 16 bytes (its registers).
struct TileModel {
    uint8_t *tile = nullptr, *pat = nullptr;
    BzfVec own[BZF_THREADS];
    TileModel()
    {
        if (posix_memalign((void **)&tile, 16, BZF_TILE + BZF_MAX_PATTERN)) abort();
        if (!(pat = (uint8_t *)malloc(BZF_MAX_PATTERN))) abort(); // (malloc aligns to more than its 4 bytes)
    }
    ~TileModel() { free(tile), free(pat); }
    // tile t of d[0, n): bzf_stage in every thread, up to the barrier
    void stage(const uint8_t *d, uint64_t n, uint64_t t, const BzfPattern &p)
    {
        memset(tile, 0xAA, BZF_TILE + BZF_MAX_PATTERN), memset(pat, 0xAA, BZF_MAX_PATTERN); // (what a thread does not store is not known)
        for (uint32_t tid = 0; tid < BZF_THREADS; tid++) own[tid] = bzf_stage(d, n, t * BZF_TILE, tid, p, tile, pat);
    }
    // behind the barrier: thread tid's hit starts among `valid`
    uint32_t match(uint32_t tid, const BzfPattern &p, uint32_t valid) const { return bzf_match16(own[tid], tid, p, tile, pat, valid); }
};

#endif // BZH_TILE_HOST_H
