// tile_host.h -- a text allocated as the kernels' contract states, for every harness that runs the tile front of
// banzai_amd/csrc/search_core.h on the host (the model of the workgroup over it: scan_host.h).
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

#endif // BZH_TILE_HOST_H
