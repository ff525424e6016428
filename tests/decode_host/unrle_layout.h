// unrle_layout.h -- the layout the inverse-RLE1 kernels of banzai_amd/csrc/decode.hip work from, for the host harnesses that run
// decode_core.h's per-thread text one thread after the other (unrle_host, pieces_host, count_host): tiles of 4,096 bytes of a
// block behind the inverse BWT, 16 a thread (what ur_load hands it), entry states by composing the threads' state maps (what
// ur_scan and unrle_walk<false> do with them), offsets by prefix sums (block_excl_add, bzp_tile_sums).  And the serial truth.
// Include decode_core.h (or a header that includes it) first.
#pragma once
#include <stdint.h>

#include <vector>

constexpr uint32_t ITEMS = BZD_UR_ITEMS, THREADS = 256, TILE = ITEMS * THREADS;

struct Thread {
    uint32_t w[4], cnt, prev, state, outn, off; // off: of its first output byte inside its tile
};
struct Tile {
    uint32_t toff, total;
    std::vector<Thread> th; // all 256, those behind the block's end with no bytes
};

// -> the state behind the block's last byte; *bsize = the block's decoded size
static uint32_t lay_out(const uint8_t *x, uint32_t n, std::vector<Tile> &tiles, uint32_t *bsize)
{
    tiles.clear();
    uint32_t pre = BZD_RL_ID, sum = 0;
    for (uint32_t t0 = 0; t0 < n; t0 += TILE) {
        Tile tl;
        tl.toff = sum;
        tl.total = 0;
        for (uint32_t i0 = t0; i0 < t0 + TILE; i0 += ITEMS) {
            Thread th = {};
            th.cnt = i0 < n ? (n - i0 < ITEMS ? n - i0 : ITEMS) : 0;
            th.prev = th.cnt && i0 ? x[i0 - 1] : 256u;
            for (uint32_t k = 0; k < th.cnt; k++) th.w[k >> 2] |= (uint32_t)x[i0 + k] << (8 * (k & 3)); // (no byte behind the block is read)
            th.state = bzd_rl_apply(pre, 0);
            pre = bzd_rl_compose(pre, bzd_ur_map(th.w, th.cnt, th.prev));
            uint32_t s_end;
            th.outn = bzd_ur_size(th.w, th.cnt, th.prev, th.state, &s_end);
            th.off = tl.total;
            tl.total += th.outn;
            tl.th.push_back(th);
        }
        sum += tl.total;
        tiles.push_back(tl);
    }
    *bsize = sum;
    return bzd_rl_apply(pre, 0);
}

// The serial inverse RLE1 of the block, libbz2's rule byte by byte: the truth.  state[i] = the state byte i is met in,
// begin[i] = where what it stands for begins in the output (begin[n] = the output's size), end = the state behind the last byte.
struct Serial {
    std::vector<uint8_t> out;
    std::vector<uint32_t> state, begin;
    uint32_t end;
};

static Serial expand(const uint8_t *x, uint32_t n)
{
    Serial r;
    r.state.resize(n);
    r.begin.resize(n + 1);
    uint32_t s = 0, prev = 256;
    for (uint32_t i = 0; i < n; i++) {
        r.state[i] = s;
        r.begin[i] = (uint32_t)r.out.size();
        if (s == 4)
            r.out.insert(r.out.end(), x[i], (uint8_t)prev);
        else
            r.out.push_back(x[i]);
        s = bzd_rl_step(s, x[i] == prev);
        prev = x[i];
    }
    r.begin[n] = (uint32_t)r.out.size();
    r.end = s;
    return r;
}
