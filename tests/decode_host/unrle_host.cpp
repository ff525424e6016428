// unrle_host.cpp -- what one thread of the decoder's random-access kernels does (banzai_amd/csrc/decode_core.h: bzd_ur_fold,
// bzd_clip, bzd_ur_emit) and the CRC algebra around it (banzai_amd/csrc/crc_gf.h), as a CPU program built by
// tests/test_index_api.py with -fsanitize=address,undefined.  The GPU kernels unrle_crc and unrle_walk_win compile the same
// text; unrle_layout.h lays the threads out as they do and this file runs them one after the other.
//
//   unrle_host <cases> <results>   cases: [u32 n][n bytes]... (a block behind the inverse BWT each)
//                                  results: [u32 crc][u32 end state][u32 len][len bytes]... (CRC from the fold, never from the bytes)
// Every case is also expanded through windows -- all of them for an expansion of at most 48 bytes, 300 seeded ones and the
// bytes around every tile seam otherwise -- each into a heap buffer of exactly the window's size, and compared with the same
// bytes of the full expansion: a byte outside the window is a sanitizer report, a wrong one exit status 1.
//
//   unrle_host --layout <cases> <dump>   what lay_out() makes of every case, for tests/unrle_paths_model.py to be held against:
//                                  [u32 tiles][u32 end state][u32 len] [u32 toff][u32 total] a tile
//                                  [u32 state][u32 outn][u32 off] a thread, 256 a tile
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../banzai_amd/csrc/crc_gf.h"
#include "../../banzai_amd/csrc/decode_core.h"
#include "unrle_layout.h"

static uint32_t g_tab[256], g_pow2[40];

static void tables()
{
    for (uint32_t i = 0; i < 256; i++) {
        uint32_t c = i << 24;
        for (int k = 0; k < 8; k++) c = (c << 1) ^ ((c >> 31) ? CRC_POLY : 0u);
        g_tab[i] = c;
    }
    uint32_t p = 2u;
    for (int k = 0; k < 40; k++) {
        g_pow2[k] = p;
        p = gf_mul(p, p);
    }
}

// unrle_crc + unrle_crc_finish
static uint32_t crc_of_expansion(const std::vector<Tile> &tiles, uint32_t bsize)
{
    uint32_t acc = 0;
    for (const Tile &tl : tiles) {
        uint32_t c = 0;
        for (const Thread &th : tl.th) {
            uint32_t outn;
            uint32_t crc = bzd_ur_fold(g_tab, th.w, th.cnt, th.prev, th.state, &outn);
            if (outn) crc = gf_mul(crc, gf_pow_x_serial(g_pow2 + 3, tl.total - th.off - outn, 20));
            c ^= crc;
        }
        acc ^= gf_mul(c, gf_pow_x_serial(g_pow2, 8ull * (bsize - tl.toff - tl.total), 40));
    }
    return acc ^ gf_mul(0xFFFFFFFFu, gf_pow_x_serial(g_pow2, 8ull * bsize, 40)) ^ 0xFFFFFFFFu;
}

// unrle_walk_win: the window [lo, hi) of the block into a buffer that holds exactly those bytes
static void expand_window(const std::vector<Tile> &tiles, uint32_t lo, uint32_t hi, std::vector<uint8_t> &out, uint32_t *tiles_walked)
{
    uint8_t *buf = (uint8_t *)malloc(hi - lo ? hi - lo : 1); // (exact size: ASan guards both ends)
    memset(buf, 0xEE, hi - lo ? hi - lo : 1);
    *tiles_walked = 0;
    for (const Tile &tl : tiles) {
        if (tl.total == 0) continue;
        uint32_t ca, cb;
        bzd_clip(tl.toff, tl.total, lo, hi, &ca, &cb);
        if (ca == cb) continue; // the tile lies outside the window
        ++*tiles_walked;
        const uint32_t tlo = ca - tl.toff, thi = cb - tl.toff;
        // g + q = where byte q of the tile belongs; it may point before the buffer, only window positions are touched
        const intptr_t g = (intptr_t)buf + ((intptr_t)tl.toff - (intptr_t)lo);
        for (const Thread &th : tl.th)
            bzd_ur_emit(th.w, th.cnt, th.prev, th.state, th.off, tlo, thi, [&](uint32_t q, uint8_t v) { *(uint8_t *)(g + (intptr_t)q) = v; });
    }
    out.assign(buf, buf + (hi - lo));
    free(buf);
}

// --layout: the tiles and threads as lay_out() places them, nothing expanded
static int dump_layout(const char *cases, const char *dump)
{
    FILE *fi = fopen(cases, "rb"), *fo = fopen(dump, "wb");
    if (!fi || !fo) return 2;
    std::vector<Tile> tiles;
    std::vector<uint32_t> words;
    for (;;) {
        uint32_t n;
        if (fread(&n, 4, 1, fi) != 1) break;
        std::vector<uint8_t> x(n ? n : 1);
        if (n && fread(x.data(), 1, n, fi) != n) return 2;
        uint32_t bsize;
        const uint32_t end = lay_out(x.data(), n, tiles, &bsize);
        words.assign({(uint32_t)tiles.size(), end, bsize});
        for (const Tile &tl : tiles) {
            words.push_back(tl.toff);
            words.push_back(tl.total);
        }
        for (const Tile &tl : tiles)
            for (const Thread &th : tl.th) {
                words.push_back(th.state);
                words.push_back(th.outn);
                words.push_back(th.off);
            }
        if (fwrite(words.data(), 4, words.size(), fo) != words.size()) return 2;
    }
    fclose(fi);
    return fclose(fo) ? 2 : 0;
}

int main(int argc, char **argv)
{
    if (argc == 4 && strcmp(argv[1], "--layout") == 0) return dump_layout(argv[2], argv[3]);
    if (argc != 3) {
        fprintf(stderr, "usage: unrle_host [--layout] <cases> <results>\n");
        return 2;
    }
    tables();
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!fi || !fo) return 2;
    uint64_t rs = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() {
        rs ^= rs << 13;
        rs ^= rs >> 7;
        rs ^= rs << 17;
        return rs;
    };
    std::vector<Tile> tiles;
    std::vector<uint8_t> full, part;
    for (long c = 0;; c++) {
        uint32_t n;
        if (fread(&n, 4, 1, fi) != 1) break;
        uint8_t *x = (uint8_t *)malloc(n ? n : 1);
        if (n && fread(x, 1, n, fi) != n) return 2;
        uint32_t bsize, walked;
        const uint32_t end = lay_out(x, n, tiles, &bsize);
        const Serial truth = expand(x, n);
        free(x);
        const uint32_t crc = crc_of_expansion(tiles, bsize);
        expand_window(tiles, 0, bsize, full, &walked);
        if (full != truth.out || end != truth.end) {
            fprintf(stderr, "unrle_host: case %ld, the layout's expansion or end state is not the serial one's\n", c);
            exit(1);
        }
        fwrite(&crc, 4, 1, fo);
        fwrite(&end, 4, 1, fo);
        fwrite(&bsize, 4, 1, fo);
        if (bsize) fwrite(full.data(), 1, bsize, fo);
        auto window = [&](uint32_t lo, uint32_t hi) {
            expand_window(tiles, lo, hi, part, &walked);
            if (part.size() != hi - lo || (hi > lo && memcmp(part.data(), full.data() + lo, hi - lo) != 0)) {
                fprintf(stderr, "unrle_host: case %ld, window [%u, %u) of %u bytes differs from the full expansion\n", c, lo, hi, bsize);
                exit(1);
            }
            uint32_t meet = 0; // tiles the window meets: no other may have been walked
            for (const Tile &tl : tiles) meet += tl.total && tl.toff < hi && tl.toff + tl.total > lo && hi > lo;
            if (walked != meet) {
                fprintf(stderr, "unrle_host: case %ld, window [%u, %u): %u tiles walked, %u meet it\n", c, lo, hi, walked, meet);
                exit(1);
            }
        };
        if (bsize <= 48) {
            for (uint32_t lo = 0; lo <= bsize; lo++)
                for (uint32_t hi = lo; hi <= bsize; hi++) window(lo, hi);
        } else {
            for (int k = 0; k < 300; k++) {
                const uint32_t lo = (uint32_t)(rnd() % (bsize + 1)), len = (uint32_t)(rnd() % (k % 3 ? 70 : 20000));
                window(lo, lo + len < bsize ? lo + len : bsize);
            }
            for (const Tile &tl : tiles) // around every tile seam, and from a seam to the block's end
                for (uint32_t d = 0; d < 5; d++) {
                    const uint32_t lo = tl.toff > 2 ? tl.toff - 2 + d : d;
                    if (lo > bsize) continue;
                    for (uint32_t len = 0; len < 6; len++) window(lo, lo + len < bsize ? lo + len : bsize);
                    window(lo, bsize);
                    window(0, lo);
                }
        }
    }
    fclose(fi);
    return fclose(fo) ? 2 : 0;
}
