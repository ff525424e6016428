// many_host.cpp -- the chain walk of bzh_decode_many (banzai_amd/csrc/decode_many_plan.h) against a restatement that judges every
// input alone and knows no batches, built with g++ -fsanitize=address,undefined.  The world is made up: a buffer is a list of
// magics with what the entropy stage -- bounded by the buffer, not by the slice -- would report at each, and what the back of
// the decoder would find for each block (size, CRC, an end in four equal bytes).  The walk is run over it in batches of every
// size from 1 on, so that a batch edge falls at every position of every chain.
//
//   many_host <seed> <cases>     exit status 0: every case held for every batch size (and the fixed ones)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <vector>

#include "../../banzai_amd/csrc/decode_many_plan.h"

static uint64_t rng_state;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}
static uint64_t below(uint64_t n) { return n ? rnd() % n : 0; }

#define CHECK(cond, ...)                                      \
    do {                                                      \
        if (!(cond)) {                                        \
            fprintf(stderr, "many_host: %s: ", #cond);        \
            fprintf(stderr, __VA_ARGS__);                     \
            fprintf(stderr, "\n");                            \
            exit(1);                                          \
        }                                                     \
    } while (0)

struct Cand { // a magic of the buffer and everything the GPU would say about it
    uint64_t pos;
    bool footer;
    BzdResult r;
    uint64_t size;    // back_sizes
    bool bad_end;
    uint32_t got_crc; // back_emit
};
enum Damage {
    D_NONE, D_KIND, D_BLOCK_CRC, D_STREAM_CRC, D_BAD_END, D_CUT_BLOCK, D_CUT_ONE_BIT, D_CUT_FOOTER, D_MAGIC, D_EMPTY, D_SHORT, D_LEVEL_FIRST,
    D_LEVEL_SECOND, D_NBLOCK, D_NO_CAND, D_NO_STREAM, D_COUNT
};
struct World {
    std::vector<Cand> cands;
    std::vector<BzmInput> in;
    std::vector<int> damage;
    std::map<uint64_t, uint32_t> headers; // byte offset of every "BZh<level>" of the buffer -> level
    uint64_t n = 0;
    int ctx_level = 5;
};

// One input at byte `off`: `nstreams` streams of 0..3 blocks with magics inside their payloads, damaged one way.  directly: the next
// input follows without a gap (so a cut block reads on into it).
static void add_input(World &w, uint64_t off, uint32_t nstreams, int dmg, bool force_one_bit)
{
    BzmInput s{};
    s.off = off;
    const uint32_t lv_ok = 1 + (uint32_t)below(w.ctx_level);
    uint64_t bit = 8 * off; // where the next thing is written
    uint64_t cut_at = 0;    // D_CUT_*: the slice ends at this bit (rounded down to a byte)
    std::vector<Cand> mine;
    if (dmg == D_EMPTY) {
        s.len = 0;
    } else if (dmg == D_SHORT) {
        s.len = 1 + below(3);
        memcpy(s.head, below(2) ? "BZh" : "BQh", 3);
    } else {
        const uint32_t dmg_stream = dmg == D_LEVEL_SECOND ? 1 : (uint32_t)below(nstreams ? nstreams : 1);
        if (dmg == D_LEVEL_SECOND && nstreams < 2) nstreams = 2;
        if (dmg == D_NO_STREAM) nstreams = 0;
        for (uint32_t q = 0; q < (nstreams ? nstreams : 1); q++) {
            uint32_t lv = lv_ok;
            if ((dmg == D_LEVEL_FIRST && q == 0) || (dmg == D_LEVEL_SECOND && q == 1)) lv = (uint32_t)w.ctx_level + 1 + (uint32_t)below(9 - w.ctx_level);
            if (q == 0) {
                memcpy(s.head, "BZh", 3);
                s.head[3] = (uint8_t)('0' + lv);
                if (dmg == D_MAGIC) s.head[below(3)] ^= 0x20;
            }
            if (!(q == 0 && dmg == D_MAGIC)) w.headers[bit / 8] = lv;
            bit += 32;
            if (!nstreams) break;
            const uint32_t nb = (uint32_t)below(4);
            uint32_t fold = 0;
            const uint32_t dmg_block = (uint32_t)below(nb ? nb : 1);
            for (uint32_t b = 0; b < nb; b++) {
                Cand c{};
                c.pos = bit;
                c.r.kind = BZD_OK;
                c.r.crc = c.got_crc = (uint32_t)rnd();
                c.r.nblock = 1 + (uint32_t)below(100000u * lv);
                c.size = 1 + below(5000);
                const uint64_t span = 90 + below(400);
                const bool hit = q == dmg_stream && b == dmg_block;
                if (hit && dmg == D_KIND) {
                    const uint32_t kinds[] = {BZD_K_TRUNC, BZD_K_FORMAT, BZD_K_RANDOMISED};
                    c.r.kind = kinds[below(3)];
                    c.r.errpos = bit + below(span);
                }
                if (hit && dmg == D_BLOCK_CRC) c.got_crc ^= 1u << below(32);
                if (hit && dmg == D_BAD_END) c.bad_end = true;
                if (hit && dmg == D_NBLOCK) c.r.nblock = 100000u * lv + 1 + (uint32_t)below(1000);
                if (hit && (dmg == D_CUT_BLOCK || dmg == D_CUT_ONE_BIT)) cut_at = bit + 48 + below(span - 48);
                fold = ((fold << 1) | (fold >> 31)) ^ c.r.crc;
                for (uint32_t o = (uint32_t)below(3); o > 0; o--) { // magics inside the payload: anything may be reported there
                    Cand x{};
                    x.pos = bit + 49 + below(span - 50);
                    x.footer = below(2);
                    x.r.kind = below(2) ? BZD_OK : BZD_K_FORMAT;
                    x.r.end_bit = x.pos + 60 + below(100000);
                    x.r.nblock = 1 + (uint32_t)below(900000);
                    x.r.follow = below(2) ? 0x109u : 2u;
                    x.size = 1 + below(5000);
                    mine.push_back(x);
                }
                bit += span;
                c.r.end_bit = bit;
                if (!(hit && dmg == D_NO_CAND)) mine.push_back(c);
            }
            Cand f{};
            f.pos = bit;
            f.footer = true;
            f.r.kind = BZD_OK;
            f.r.crc = fold;
            const bool here = q == dmg_stream;
            if (here && dmg == D_STREAM_CRC) f.r.crc ^= 1u << below(32);
            if (here && (dmg == D_CUT_FOOTER || ((dmg == D_CUT_BLOCK || dmg == D_CUT_ONE_BIT) && nb == 0))) cut_at = bit + 48 + below(32);
            bit = (bit + 80 + 7) / 8 * 8;
            f.r.end_bit = bit; // (follow is filled in once the buffer is laid out)
            if (!(here && dmg == D_NO_CAND && nb == 0)) mine.push_back(f); // (no block to lose: the footer's magic is lost instead)
        }
        s.len = (bit + 7) / 8 - off;
        if (cut_at) {
            if (force_one_bit || dmg == D_CUT_ONE_BIT) { // the cut block ends ONE bit behind the slice
                const uint64_t hi = cut_at / 8 * 8;
                for (Cand &c : mine)
                    if (c.pos < hi && c.r.end_bit > hi && c.r.kind == BZD_OK && c.pos + 48 <= hi && !c.footer) c.r.end_bit = hi + 1;
            }
            s.len = cut_at / 8 - off;
        }
    }
    const uint64_t hi = 8 * (s.off + s.len);
    for (auto it = w.headers.lower_bound(s.off); it != w.headers.end();) // headers behind the cut are not in the buffer
        it = it->first * 8 + 32 > hi ? w.headers.erase(it) : ++it;
    for (Cand &c : mine) {
        if (c.pos + 48 > hi) continue; // its magic is not in the buffer
        w.cands.push_back(c);
    }
    w.in.push_back(s);
    w.damage.push_back(dmg);
}

static World make_world(size_t inputs, int only_damage, bool all_damaged, bool one_bit)
{
    World w;
    w.ctx_level = 1 + (int)below(9);
    if (w.ctx_level == 9) w.ctx_level = 8; // (room for a level above it)
    uint64_t off = below(3) ? 0 : below(40);
    for (size_t k = 0; k < inputs; k++) {
        int dmg = only_damage >= 0 ? only_damage : (all_damaged || below(3) == 0) ? 1 + (int)below(D_COUNT - 1) : D_NONE;
        add_input(w, off, (uint32_t)below(4), dmg, one_bit);
        off = w.in.back().off + w.in.back().len;
        if (below(2)) { // a gap, with a magic in it now and then
            const uint64_t gap = 1 + below(30);
            if (gap >= 8 && below(2)) {
                Cand x{};
                x.pos = 8 * off + below(8 * gap - 48);
                x.footer = below(2);
                x.r.kind = BZD_OK;
                x.r.end_bit = x.pos + 80 + below(5000);
                x.r.nblock = 1 + (uint32_t)below(1000);
                x.size = 1 + below(100);
                w.cands.push_back(x);
            }
            off += gap;
        }
    }
    w.n = off;
    std::sort(w.cands.begin(), w.cands.end(), [](const Cand &a, const Cand &b) { return a.pos < b.pos; });
    // what the kernel reports behind a footer: it looks at the BUFFER
    for (Cand &c : w.cands) {
        if (!c.footer) continue;
        const uint64_t end = c.r.end_bit / 8;
        if (end > w.n) {
            c.r.kind = BZD_K_TRUNC;
            c.r.errpos = w.n * 8;
            continue;
        }
        c.r.follow = end == w.n ? 0u : 2u;
        auto it = w.headers.find(end);
        if (it != w.headers.end() && end + 4 <= w.n) c.r.follow = 0x100u | it->second;
    }
    // a block cut by its slice reads on: whatever it reports ends behind the slice (or it fails)
    return w;
}

struct Verdict {
    int status;
    uint64_t consumed_max, out_len, decoded;
    std::vector<uint64_t> footer_ends; // consumed of a failed input is one of these, or 0
};

// input k judged alone: bzh_decode's rules over the slice, candidate by candidate, no batches.  With one damage an input its
// status does not depend on which of two failures is found first.
static Verdict alone(const World &w, size_t k)
{
    const BzmInput &s = w.in[k];
    Verdict v{BZM_OK, 0, 0, 0, {}};
    if (s.len < 4 || s.head[0] != 'B' || s.head[1] != 'Z' || s.head[2] != 'h' || s.head[3] < '1' || s.head[3] > '9') {
        v.status = BZM_E_DATA;
        return v;
    }
    uint32_t level = s.head[3] - '0';
    if ((int)level > w.ctx_level) {
        v.status = BZM_E_ARG;
        return v;
    }
    const uint64_t lo = 8 * s.off, hi = 8 * (s.off + s.len);
    uint64_t pos = lo + 32;
    uint32_t fold = 0;
    bool back_failed = false; // a failure the back of the decoder finds: the walk itself goes on to the end of the batch
    for (;;) {
        const Cand *c = nullptr;
        for (const Cand &x : w.cands)
            if (x.pos == pos && x.pos + 48 <= hi) c = &x;
        if (!c || c->r.kind != BZD_OK || c->r.end_bit > hi) break;
        if (!c->footer) {
            if (c->r.nblock > 100000u * level) break;
            if (c->bad_end || c->got_crc != c->r.crc) back_failed = true;
            fold = ((fold << 1) | (fold >> 31)) ^ c->r.crc;
            v.decoded += c->size;
            pos = c->r.end_bit;
            continue;
        }
        v.consumed_max = c->r.end_bit / 8 - s.off;
        v.footer_ends.push_back(v.consumed_max);
        if (fold != c->r.crc) back_failed = true;
        fold = 0;
        const uint64_t end = c->r.end_bit / 8;
        auto it = w.headers.find(end);
        if (it != w.headers.end() && end + 4 <= s.off + s.len) { // the next stream, inside the slice
            level = it->second;
            if ((int)level > w.ctx_level) {
                v.status = back_failed ? BZM_E_DATA : BZM_E_ARG;
                return v;
            }
            pos = c->r.end_bit + 32;
            continue;
        }
        v.status = back_failed ? BZM_E_DATA : BZM_OK;
        v.out_len = v.decoded;
        return v;
    }
    v.status = BZM_E_DATA;
    return v;
}

static void run_case(const World &w, uint32_t max_batch)
{
    std::vector<uint64_t> cl;
    for (const Cand &c : w.cands) cl.push_back(c.pos << 1 | (c.footer ? 1 : 0));
    BzmWalk walk;
    walk.cands = cl.data();
    walk.nc = cl.size();
    walk.in = w.in.data();
    walk.count = w.in.size();
    walk.ctx_level = w.ctx_level;
    walk.start();
    size_t first;
    uint32_t B;
    size_t batches = 0, given = 0;
    while (walk.next_batch(max_batch, &first, &B)) {
        CHECK(B >= 1 && B <= max_batch && first + B <= cl.size() && first >= given, "batch [%zu, +%u) of %zu", first, B, cl.size());
        given = first + B;
        std::vector<BzdResult> res(B); // exactly the batch: one slot further is a report
        for (uint32_t q = 0; q < B; q++) res[q] = w.cands[first + q].r;
        walk.feed(res.data());
        for (BzmItem &it : walk.items) {
            CHECK(it.slot < B, "slot %u of %u", it.slot, B);
            if (it.footer || it.dead) continue;
            it.size = w.cands[first + it.slot].size;
            it.bad_end = w.cands[first + it.slot].bad_end;
        }
        walk.place(UINT64_MAX);
        for (BzmItem &it : walk.items)
            if (it.placed) it.got_crc = w.cands[first + it.slot].got_crc;
        walk.check(true);
        batches++;
        CHECK(batches <= cl.size() + 1, "the walk does not end");
    }
    walk.finish();
    uint64_t at = 0;
    for (size_t k = 0; k < w.in.size(); k++) {
        const Verdict v = alone(w, k);
        const BzmState &s = walk.st[k];
        CHECK(s.status == v.status, "input %zu of %zu (damage %d, batch %u): status %d, alone %d", k, w.in.size(), w.damage[k], max_batch, s.status, v.status);
        CHECK(s.off_set && s.out_off == at, "input %zu: out_off %llu, the output stood at %llu", k, (unsigned long long)s.out_off, (unsigned long long)at);
        if (v.status == BZM_OK) {
            CHECK(s.out_len == v.out_len, "input %zu: out_len %llu, alone %llu", k, (unsigned long long)s.out_len, (unsigned long long)v.out_len);
            CHECK(s.consumed == v.consumed_max, "input %zu: consumed %llu, alone %llu", k, (unsigned long long)s.consumed, (unsigned long long)v.consumed_max);
            at = s.out_off + s.out_len;
        } else {
            CHECK(s.out_len == 0, "input %zu failed with out_len %llu", k, (unsigned long long)s.out_len);
            CHECK(s.decoded <= v.decoded, "input %zu: a gap of %llu bytes, it decodes %llu at most", k, (unsigned long long)s.decoded, (unsigned long long)v.decoded);
            CHECK(s.consumed == 0 || std::find(v.footer_ends.begin(), v.footer_ends.end(), s.consumed) != v.footer_ends.end(),
                  "input %zu: consumed %llu is the end of no stream of it", k, (unsigned long long)s.consumed);
            // behind a failed input the next one starts behind the gap, and the gap is at most what it had decoded
            const uint64_t next = k + 1 < w.in.size() ? walk.st[k + 1].out_off : walk.total_out;
            CHECK(next >= s.out_off && next - s.out_off == s.decoded, "input %zu: gap %llu, placed %llu", k, (unsigned long long)(next - s.out_off),
                  (unsigned long long)s.decoded);
            at = next;
        }
    }
    CHECK(at == walk.total_out, "the output ends at %llu, the inputs at %llu", (unsigned long long)walk.total_out, (unsigned long long)at);
    CHECK(walk.off_chain <= cl.size(), "off-chain count");
}

static void run_world(const World &w)
{
    for (uint32_t mb : {1u, 2u, 3u, 4u, 5u, 7u, 8u, 16u, 1000u}) run_case(w, mb);
}

int main(int argc, char **argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: many_host <seed> <cases>\n");
        return 2;
    }
    rng_state = strtoull(argv[1], nullptr, 10) * 0x9E3779B97F4A7C15ull + 1;
    const size_t cases = strtoull(argv[2], nullptr, 10);
    for (int d = 0; d < D_COUNT; d++) // every damage alone, then every input damaged that way
        for (int rep = 0; rep < 20; rep++) {
            run_world(make_world(1, d, false, false));
            run_world(make_world(1 + below(6), d, false, rep & 1));
        }
    for (int rep = 0; rep < 50; rep++) run_world(make_world(1 + below(12), -1, true, false)); // every input failed
    run_world(make_world(0, -1, false, false));
    for (size_t c = 0; c < cases; c++) run_world(make_world(1 + below(10), -1, false, below(4) == 0));
    printf("many_host: %zu cases held for every batch size\n", cases);
    return 0;
}
