// bzd_host.cpp -- the decoder's serial front (banzai_amd/csrc/decode_core.h) as a one-lane CPU program, built by
// tests/test_decode_host.py with -fsanitize=address,undefined.  The GPU kernel compiles the same header; here damaged streams
// can be thrown at it freely.  Around the shared parser this file supplies what the GPU does in other kernels, serially: the
// chain from block to block, the inverse BWT, the inverse RLE1 (twice: libbz2's loop, and the state-map model the GPU scans
// with -- they must agree) and the CRCs.
//
//   bzd_host decode <cases> <results>   cases: [u32 n][n bytes]...  results: [i32 kind][u64 consumed][u64 len][len bytes]...
//   bzd_host rlemodel <seed> <count>    random blocks over a small alphabet: model against loop; exit status 1 on a difference
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../banzai_amd/csrc/decode_core.h"

static uint32_t crc_table[256];
static void crc_init()
{
    for (uint32_t i = 0; i < 256; i++) {
        uint32_t c = i << 24;
        for (int k = 0; k < 8; k++) c = (c & 0x80000000u) ? (c << 1) ^ 0x04C11DB7u : (c << 1);
        crc_table[i] = c;
    }
}

// libbz2's rule, serially: four equal bytes, then a count byte.  false: the block ends in four equal bytes without a count.
static bool unrle_loop(const uint8_t *x, size_t n, std::vector<uint8_t> &out)
{
    int same = 0, prev = -1;
    for (size_t i = 0; i < n; i++) {
        const uint8_t b = x[i];
        if (same == 4) {
            out.insert(out.end(), b, (uint8_t)prev);
            same = 0;
            prev = -1;
            continue;
        }
        if ((int)b == prev) {
            same++;
        } else {
            same = 1;
            prev = b;
        }
        out.push_back(b);
    }
    return same != 4;
}

// The model the GPU runs: a state map per 16-byte chunk, the maps composed in order (there: a scan), and every chunk walked
// from the state the composition hands it.
static bool unrle_model(const uint8_t *x, size_t n, std::vector<uint8_t> &out, size_t chunk = 16)
{
    const size_t nchunks = (n + chunk - 1) / chunk;
    std::vector<uint32_t> maps(nchunks);
    for (size_t c = 0; c < nchunks; c++) {
        uint32_t st[5] = {0, 1, 2, 3, 4};
        for (size_t i = c * chunk; i < n && i < (c + 1) * chunk; i++)
            for (int s = 0; s < 5; s++) st[s] = bzd_rl_step(st[s], i > 0 && x[i] == x[i - 1]);
        maps[c] = st[0] | st[1] << 3 | st[2] << 6 | st[3] << 9 | st[4] << 12;
    }
    uint32_t pre = BZD_RL_ID, s = 0;
    for (size_t c = 0; c < nchunks; c++) {
        s = bzd_rl_apply(pre, 0);
        for (size_t i = c * chunk; i < n && i < (c + 1) * chunk; i++) {
            if (s == 4)
                out.insert(out.end(), x[i], x[i - 1]);
            else
                out.push_back(x[i]);
            s = bzd_rl_step(s, i > 0 && x[i] == x[i - 1]);
        }
        pre = bzd_rl_compose(pre, maps[c]);
    }
    return bzd_rl_apply(pre, 0) != 4;
}

struct Decoded {
    uint32_t kind = 0;
    uint64_t consumed = 0;
    std::vector<uint8_t> out;
};

static BzdWork g_work;

static uint64_t peek48(const uint8_t *in, uint64_t n, uint64_t pos)
{
    BzdBits r;
    bzd_seek(r, in, n, pos);
    const uint64_t hi = bzd_get(r, 24);
    return hi << 24 | bzd_get(r, 24);
}

static void decode(const uint8_t *in, uint64_t n, Decoded &d)
{
    d = Decoded();
    uint64_t at = 0; // byte where the current stream starts
    size_t streams = 0;
    std::vector<uint8_t> L(900000), blk(900000), raw, raw2;
    std::vector<uint32_t> tt(900000);
    for (;;) {
        if (n - at < 4) {
            d.kind = (n - at) && memcmp(in + at, "BZh", n - at < 3 ? n - at : 3) != 0 ? BZD_K_MAGIC : BZD_K_TRUNC;
            return;
        }
        if (in[at] != 'B' || in[at + 1] != 'Z' || in[at + 2] != 'h' || in[at + 3] < '1' || in[at + 3] > '9') {
            d.kind = BZD_K_MAGIC;
            return;
        }
        const uint32_t block_max = 100000u * (uint32_t)(in[at + 3] - '0');
        uint64_t pos = at * 8 + 32;
        uint32_t stream_crc = 0;
        for (;;) {
            if (pos + 48 > n * 8) {
                d.kind = BZD_K_TRUNC;
                return;
            }
            const uint64_t magic = peek48(in, n, pos);
            BzdResult r;
            if (magic == BZD_FOOTER_MAGIC) {
                bzd_parse_footer(in, n, pos, r);
                if (r.kind) {
                    d.kind = r.kind;
                    return;
                }
                if (r.crc != stream_crc) {
                    d.kind = BZD_K_STREAM_CRC;
                    return;
                }
                streams++;
                d.consumed = r.end_bit / 8;
                if (!(r.follow & 0x100u)) return; // the end of the input, or foreign bytes
                at = r.end_bit / 8;
                break;
            }
            if (magic != BZD_BLOCK_MAGIC) {
                d.kind = BZD_K_MAGIC;
                return;
            }
            bzd_decode_block(g_work, in, n, pos, block_max, L.data(), r);
            if (r.kind) {
                d.kind = r.kind;
                return;
            }
            // inverse BWT
            const uint32_t nb = r.nblock;
            uint32_t cf[257] = {0};
            for (uint32_t i = 0; i < nb; i++) cf[L[i] + 1]++;
            for (int k = 0; k < 256; k++) cf[k + 1] += cf[k];
            for (uint32_t i = 0; i < nb; i++) tt[cf[L[i]]++] = i;
            uint32_t tpos = tt[r.origptr];
            for (uint32_t i = 0; i < nb; i++) {
                blk[i] = L[tpos];
                tpos = tt[tpos];
            }
            raw.clear();
            raw2.clear();
            const bool ok = unrle_loop(blk.data(), nb, raw), ok2 = unrle_model(blk.data(), nb, raw2);
            if (ok != ok2 || raw != raw2) {
                fprintf(stderr, "bzd_host: the state-map model of the inverse RLE1 differs from the loop\n");
                exit(3);
            }
            if (!ok) {
                d.kind = BZD_K_FORMAT;
                return;
            }
            uint32_t crc = 0xFFFFFFFFu;
            for (uint8_t b : raw) crc = (crc << 8) ^ crc_table[(crc >> 24) ^ b];
            crc = ~crc;
            if (crc != r.crc) {
                d.kind = BZD_K_BLOCK_CRC;
                return;
            }
            stream_crc = ((stream_crc << 1) | (stream_crc >> 31)) ^ crc;
            d.out.insert(d.out.end(), raw.begin(), raw.end());
            pos = r.end_bit;
        }
    }
}

static int run_decode(const char *cases, const char *results)
{
    FILE *fi = fopen(cases, "rb"), *fo = fopen(results, "wb");
    if (!fi || !fo) return 2;
    std::vector<uint8_t> buf;
    Decoded d;
    for (;;) {
        uint32_t n;
        if (fread(&n, 4, 1, fi) != 1) break;
        // an exact-size heap copy: a read one byte past the case is a sanitizer report, not a lucky zero
        uint8_t *in = (uint8_t *)malloc(n ? n : 1);
        if (n && fread(in, 1, n, fi) != n) return 2;
        decode(in, n, d);
        free(in);
        const int32_t kind = (int32_t)d.kind;
        const uint64_t consumed = d.kind ? 0 : d.consumed, len = d.kind ? 0 : d.out.size();
        fwrite(&kind, 4, 1, fo);
        fwrite(&consumed, 8, 1, fo);
        fwrite(&len, 8, 1, fo);
        if (len) fwrite(d.out.data(), 1, len, fo);
    }
    fclose(fi);
    return fclose(fo) ? 2 : 0;
}

static int run_rlemodel(uint64_t seed, long count)
{
    static const uint8_t alphabet[5] = {0, 1, 4, 5, 255};
    uint64_t s = seed * 0x9E3779B97F4A7C15ull + 1;
    auto rnd = [&]() {
        s ^= s << 13;
        s ^= s >> 7;
        s ^= s << 17;
        return s;
    };
    std::vector<uint8_t> x, a, b;
    for (long c = 0; c < count; c++) {
        const size_t n = 1 + rnd() % 96;
        const uint32_t stick = (uint32_t)(rnd() % 4); // how much the bytes like to repeat
        x.resize(n);
        for (size_t i = 0; i < n; i++) x[i] = (i && rnd() % 4 < stick) ? x[i - 1] : alphabet[rnd() % 5];
        a.clear();
        b.clear();
        const size_t chunk = 1 + rnd() % 20;
        const bool ok = unrle_loop(x.data(), n, a), ok2 = unrle_model(x.data(), n, b, chunk);
        if (ok != ok2 || a != b) {
            fprintf(stderr, "rlemodel: case %ld (n = %zu, chunk = %zu) differs\n", c, n, chunk);
            return 1;
        }
    }
    return 0;
}

int main(int argc, char **argv)
{
    crc_init();
    if (argc == 4 && !strcmp(argv[1], "decode")) return run_decode(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "rlemodel")) return run_rlemodel(strtoull(argv[2], nullptr, 10), atol(argv[3]));
    fprintf(stderr, "usage: bzd_host decode <cases> <results> | bzd_host rlemodel <seed> <count>\n");
    return 2;
}
