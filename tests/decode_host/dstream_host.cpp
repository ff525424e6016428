// dstream_host.cpp -- the resumable chain walk and the feed loop of bzh_dstream_* (banzai_amd/csrc/decode_stream_plan.h) against a
// restatement that walks the whole buffer once and knows no windows, built with g++ -fsanitize=address,undefined.  The world is
// made up: an input is real bytes only where the walk reads bytes (the stream headers, the tail), and otherwise a list of magics
// with what the entropy stage would report at each when the input ended at a given byte, and what the back of the decoder would
// find for each block (size, CRC, an end in four equal bytes).  The device is a fake that keeps a real window and a real staging
// buffer, so every append, move, grow and hand-out is checked byte by byte against the input and the expected output.
//
//   dstream_host <seed> <cases>     exit status 0: every case held for every chunking and room, and every path was reached
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../banzai_amd/csrc/decode_stream_plan.h"

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
            fprintf(stderr, "dstream_host: %s: ", #cond);     \
            fprintf(stderr, __VA_ARGS__);                     \
            fprintf(stderr, "\n");                            \
            exit(1);                                          \
        }                                                     \
    } while (0)

struct Item { // a magic of the input and everything the GPU would say about it
    uint64_t pos;
    bool footer, on_chain;
    uint64_t end_bit;  // block: its natural end
    uint32_t kind;     // block: a defect the parse finds at errpos (BZD_OK: none)
    uint64_t errpos;
    uint32_t crc, nblock;
    uint64_t size;
    bool bad_end;
    uint32_t got_crc;
    uint32_t id;
    BzdResult off; // off the chain: anything
};
enum Damage {
    D_NONE, D_FORMAT, D_RANDOMISED, D_BLOCK_CRC, D_STREAM_CRC, D_BAD_END, D_NBLOCK, D_CUT, D_HEAD_MAGIC, D_LOST_MAGIC, D_LEVEL_FIRST, D_LEVEL_LATER,
    D_EMPTY_INPUT, D_SHORT_INPUT, D_COUNT
};
struct World {
    std::vector<uint8_t> in; // N bytes
    std::vector<Item> items; // ascending
    int ctx_level = 5;
    int damage = D_NONE;
};

static uint8_t filler(uint64_t i) { return (uint8_t)(0x80u | ((i * 131u + 7u) & 0x7Fu)); } // (never a letter of "BZh1")
static uint8_t out_byte(uint32_t id, uint64_t j) { return (uint8_t)(id * 37u + j * 11u + 3u); }

static World make_world(int dmg)
{
    World w;
    w.damage = dmg;
    std::vector<uint8_t> &in = w.in;
    auto put = [&](uint64_t at, const char *s, size_t n) {
        while (in.size() < at + n) in.push_back(filler(in.size()));
        for (size_t k = 0; k < n; k++) in[at + k] = (uint8_t)s[k];
    };
    if (dmg == D_EMPTY_INPUT) return w;
    if (dmg == D_SHORT_INPUT) {
        const char *s = below(2) ? "BZh" : "BQh";
        put(0, s, 1 + below(3));
        return w;
    }
    uint32_t nstreams = 1 + (uint32_t)below(5);
    if (dmg == D_LEVEL_LATER && nstreams < 2) nstreams = 2;
    const uint32_t dmg_stream = dmg == D_LEVEL_LATER ? 1 + (uint32_t)below(nstreams - 1) : dmg == D_LEVEL_FIRST || dmg == D_HEAD_MAGIC ? 0 : (uint32_t)below(nstreams);
    uint64_t bit = 0;
    uint32_t id = 0;
    std::vector<uint64_t> block_bits; // D_CUT: where the input may be cut
    for (uint32_t q = 0; q < nstreams; q++) {
        uint32_t lv = 1 + (uint32_t)below(w.ctx_level);
        if ((dmg == D_LEVEL_FIRST || dmg == D_LEVEL_LATER) && q == dmg_stream) lv = (uint32_t)w.ctx_level + 1 + (uint32_t)below(9 - w.ctx_level);
        char h[4] = {'B', 'Z', 'h', (char)('0' + lv)};
        if (dmg == D_HEAD_MAGIC && q == 0) h[below(4)] ^= 0x40;
        put(bit / 8, h, 4);
        bit += 32;
        uint32_t nb = (uint32_t)below(7);
        const bool needs_block = dmg == D_FORMAT || dmg == D_RANDOMISED || dmg == D_BLOCK_CRC || dmg == D_BAD_END || dmg == D_NBLOCK;
        if (needs_block && q == dmg_stream && nb == 0) nb = 1;
        const uint32_t dmg_block = (uint32_t)below(nb ? nb : 1);
        uint32_t fold = 0;
        for (uint32_t b = 0; b <= nb; b++) { // the blocks, then the footer
            const bool hit = q == dmg_stream && b == dmg_block;
            Item c{};
            c.pos = bit;
            c.on_chain = true;
            c.id = id++;
            if (b == nb) {
                c.footer = true;
                c.crc = fold;
                if (dmg == D_STREAM_CRC && q == dmg_stream) c.crc ^= 1u << below(32);
                if (!(dmg == D_LOST_MAGIC && q == dmg_stream && nb == 0)) w.items.push_back(c);
                block_bits.push_back(bit + below(80));
                bit = (bit + 80 + 7) / 8 * 8;
                break;
            }
            const uint64_t span = 90 + below(400);
            c.end_bit = bit + span;
            c.crc = c.got_crc = (uint32_t)rnd();
            c.nblock = 1 + (uint32_t)below(100000u * lv);
            c.size = 1 + below(300);
            if (hit && (dmg == D_FORMAT || dmg == D_RANDOMISED)) {
                c.kind = dmg == D_FORMAT ? BZD_K_FORMAT : BZD_K_RANDOMISED;
                c.errpos = bit + 48 + below(span - 48);
            }
            if (hit && dmg == D_BLOCK_CRC) c.got_crc ^= 1u << below(32);
            if (hit && dmg == D_BAD_END) c.bad_end = true;
            if (hit && dmg == D_NBLOCK) c.nblock = 100000u * lv + 1 + (uint32_t)below(1000);
            fold = ((fold << 1) | (fold >> 31)) ^ c.crc;
            if (!(hit && dmg == D_LOST_MAGIC)) w.items.push_back(c);
            block_bits.push_back(bit + below(span));
            for (uint32_t o = (uint32_t)below(3); o > 0; o--) { // magics inside the payload: anything may be reported there
                Item x{};
                x.pos = bit + 49 + below(span - 50);
                x.footer = below(2);
                x.id = id++;
                x.off.kind = below(2) ? BZD_OK : BZD_K_FORMAT;
                x.off.end_bit = x.pos + 60 + below(100000);
                x.off.nblock = 1 + (uint32_t)below(900000);
                x.off.follow = below(2) ? 0x109u : 2u;
                w.items.push_back(x);
            }
            bit = c.end_bit;
        }
    }
    while (in.size() < bit / 8) in.push_back(filler(in.size()));
    switch (below(4)) { // the tail
    case 0: break;
    case 1: put(in.size(), "\x01\x02\x03", 3); break;                // foreign
    case 2: put(in.size(), "BZh", 1 + below(3)); break;              // a prefix of "BZh9"
    default: put(in.size(), "BZhx and more foreign bytes", 5 + below(20)); break;
    }
    if (dmg == D_CUT) in.resize((size_t)(block_bits[below(block_bits.size())] / 8));
    std::sort(w.items.begin(), w.items.end(), [](const Item &a, const Item &b) { return a.pos < b.pos; });
    // (two magics at one bit cannot be: an off-chain one that fell on another's position moves on)
    for (size_t k = 1; k < w.items.size(); k++)
        if (w.items[k].pos <= w.items[k - 1].pos) w.items[k].pos = w.items[k - 1].pos + 1;
    return w;
}

// What the entropy stage reports of an item when the bytes it sees end at byte E (absolute coordinates).  bytes: the input from
// byte `base` on, `E - base` of them.
static BzdResult truth(const Item &c, uint64_t E, const uint8_t *bytes, uint64_t base)
{
    if (!c.on_chain) return c.off;
    BzdResult r{};
    r.crc = c.crc;
    if (!c.footer) {
        if (c.kind != BZD_OK && c.errpos <= 8 * E) {
            r.kind = c.kind;
            r.errpos = c.errpos;
        } else if (c.end_bit > 8 * E) {
            r.kind = BZD_K_TRUNC;
            r.errpos = 8 * E;
        } else {
            r.end_bit = c.end_bit;
            r.nblock = c.nblock;
        }
        return r;
    }
    const uint64_t end = (c.pos + 80 + 7) / 8;
    r.end_bit = end * 8;
    if (c.pos + 80 > 8 * E) {
        r.kind = BZD_K_TRUNC;
        r.errpos = 8 * E;
        return r;
    }
    if (end == E) return r;
    r.follow = 2;
    if (end + 4 <= E) {
        const uint8_t *h = bytes + (end - base);
        if (h[0] == 'B' && h[1] == 'Z' && h[2] == 'h' && h[3] >= '1' && h[3] <= '9') r.follow = 0x100u | (uint32_t)(h[3] - '0');
    }
    return r;
}

struct Verdict {
    int status = BZS_OK;
    BzsError err{};
    uint64_t consumed = 0;
    std::vector<uint8_t> out; // of the blocks in front of the defect
};

// The restatement: the whole input, one walk, item by item.
static Verdict judge(const World &w)
{
    Verdict v;
    const uint64_t N = w.in.size(), nbits = 8 * N;
    auto fail = [&](int st, uint32_t kind, uint64_t bit, size_t s, size_t b, const char *what, uint32_t lv = 0) {
        v.status = st;
        v.err = BzsError{kind, lv, bit, s, b, what};
        return v;
    };
    if (N < 4) return fail(BZS_E_DATA, N && memcmp(w.in.data(), "BZh", N < 3 ? (size_t)N : 3) != 0 ? BZD_K_MAGIC : BZD_K_TRUNC, N * 8, 0, 0, "no stream header");
    const uint8_t *h = w.in.data();
    if (h[0] != 'B' || h[1] != 'Z' || h[2] != 'h' || h[3] < '1' || h[3] > '9') return fail(BZS_E_DATA, BZD_K_MAGIC, 0, 0, 0, "no \"BZh1\"..\"BZh9\"");
    uint32_t lv = (uint32_t)(h[3] - '0'), fold = 0;
    if ((int)lv > w.ctx_level) return fail(BZS_E_ARG, BZD_OK, 0, 0, 0, nullptr, lv);
    uint64_t pos = 32;
    size_t s = 0, b = 0;
    for (;;) {
        const Item *c = nullptr;
        for (const Item &x : w.items)
            if (x.pos == pos && x.pos + 48 <= nbits) c = &x;
        if (!c) return fail(BZS_E_DATA, pos + 48 > nbits ? BZD_K_TRUNC : BZD_K_MAGIC, pos, s, b, "neither a block nor a footer");
        const BzdResult r = truth(*c, N, w.in.data(), 0);
        if (r.kind != BZD_OK) return fail(BZS_E_DATA, r.kind, r.errpos, s, b, nullptr);
        if (!c->footer) {
            if (r.nblock > 100000u * lv) return fail(BZS_E_DATA, BZD_K_FORMAT, pos, s, b, "more bytes than the stream's block size");
            if (c->bad_end) return fail(BZS_E_DATA, BZD_K_FORMAT, pos, s, b, "the block ends in four equal bytes without a count");
            if (c->got_crc != c->crc) return fail(BZS_E_DATA, BZD_K_BLOCK_CRC, pos, s, b, nullptr);
            for (uint64_t j = 0; j < c->size; j++) v.out.push_back(out_byte(c->id, j));
            fold = ((fold << 1) | (fold >> 31)) ^ c->crc;
            b++;
            pos = r.end_bit;
            continue;
        }
        v.consumed = r.end_bit / 8;
        if (fold != c->crc) return fail(BZS_E_DATA, BZD_K_STREAM_CRC, pos, s, b, nullptr);
        fold = 0;
        if (!(r.follow & 0x100u)) return v;
        s++;
        b = 0;
        lv = r.follow & 15u;
        if ((int)lv > w.ctx_level) return fail(BZS_E_ARG, BZD_OK, 0, s, 0, nullptr, lv);
        pos = r.end_bit + 32;
    }
}

// The fake device: a real window and a real staging buffer, sized exactly, so that the sanitizer sees every byte out of place.
struct FakeDev {
    const World *w = nullptr;
    const BzsStream<FakeDev> *walk = nullptr;
    uint32_t batch = 1000;
    std::vector<uint8_t> win, staging;
    std::vector<const Item *> slot_item;

    uint32_t max_batch() const { return batch; }
    void check_window(uint64_t held) const
    {
        CHECK(held <= win.size(), "%llu bytes held in a window of %zu", (unsigned long long)held, win.size());
        for (uint64_t j = 0; j < held; j++)
            CHECK(win[j] == w->in[walk->base + j], "window byte %llu is not input byte %llu", (unsigned long long)j, (unsigned long long)(walk->base + j));
    }
    int win_reserve(uint64_t cap, uint64_t keep)
    {
        CHECK(keep <= win.size() && keep <= cap, "keep %llu of %zu into %llu", (unsigned long long)keep, win.size(), (unsigned long long)cap);
        std::vector<uint8_t> nw(cap);
        std::copy(win.begin(), win.begin() + (ptrdiff_t)keep, nw.begin());
        win.swap(nw);
        return 0;
    }
    int win_append(uint64_t at, const uint8_t *src, uint64_t n)
    {
        CHECK(at + n <= win.size(), "append [%llu, +%llu) to a window of %zu", (unsigned long long)at, (unsigned long long)n, win.size());
        memcpy(win.data() + at, src, n);
        return 0;
    }
    int win_move(uint64_t from, uint64_t len)
    {
        CHECK(from + len <= win.size() && from > 0 && len > 0, "move [%llu, +%llu) of %zu", (unsigned long long)from, (unsigned long long)len, win.size());
        std::vector<uint8_t> nw(win.size()); // (another buffer, as the real device has)
        memcpy(nw.data(), win.data() + from, len);
        win.swap(nw);
        return 0;
    }
    int scan(uint64_t from, uint64_t to, std::vector<uint64_t> &hits)
    {
        check_window(to);
        hits.clear();
        const uint64_t lo = 8 * (walk->base + from), hi = 8 * (walk->base + to);
        for (const Item &c : w->items)
            if (c.pos >= lo && c.pos + 48 <= hi) hits.push_back((c.pos - 8 * walk->base) << 1 | (c.footer ? 1ull : 0ull));
        return 0;
    }
    int entropy(const uint64_t *cands, uint32_t B, uint64_t held, BzdResult *res)
    {
        check_window(held);
        CHECK(B >= 1 && B <= batch, "a batch of %u", B);
        slot_item.assign(B, nullptr);
        for (uint32_t k = 0; k < B; k++) {
            const uint64_t pos = (cands[k] >> 1) + 8 * walk->base;
            CHECK(k == 0 || cands[k] > cands[k - 1], "candidates not ascending");
            const Item *c = nullptr;
            for (const Item &x : w->items)
                if (x.pos == pos) c = &x;
            CHECK(c && c->footer == ((cands[k] & 1ull) != 0) && pos + 48 <= 8 * (walk->base + held), "candidate %u is no magic of the window", k);
            slot_item[k] = c;
            BzdResult r = truth(*c, walk->base + held, win.data(), walk->base);
            r.errpos -= 8 * walk->base; // window coordinates
            r.end_bit -= 8 * walk->base;
            res[k] = r;
        }
        return 0;
    }
    int sizes(std::vector<BzsBlock> &blocks, uint32_t Bu, uint32_t nmax_all)
    {
        CHECK(Bu <= slot_item.size() && nmax_all >= 1, "slots up to %u of %zu", Bu, slot_item.size());
        for (BzsBlock &b : blocks) {
            CHECK(b.slot < Bu && !slot_item[b.slot]->footer && slot_item[b.slot]->on_chain, "slot %u is no block of the chain", b.slot);
            CHECK(b.nblock == slot_item[b.slot]->nblock && b.nblock <= nmax_all, "nblock of slot %u", b.slot);
            b.size = slot_item[b.slot]->size;
            b.bad_end = slot_item[b.slot]->bad_end;
        }
        return 0;
    }
    int stage_reserve(uint64_t cap)
    {
        staging.assign(cap, 0xEE);
        return 0;
    }
    int emit(std::vector<BzsBlock> &blocks, size_t taken)
    {
        CHECK(taken >= 1 && taken <= blocks.size(), "%zu of %zu blocks taken", taken, blocks.size());
        for (size_t q = 0; q < taken; q++) {
            const Item *c = slot_item[blocks[q].slot];
            CHECK(blocks[q].base + c->size <= staging.size(), "block %zu at %llu + %llu in a staging buffer of %zu", q,
                  (unsigned long long)blocks[q].base, (unsigned long long)c->size, staging.size());
            for (uint64_t j = 0; j < c->size; j++) staging[blocks[q].base + j] = out_byte(c->id, j);
            blocks[q].crc = c->got_crc;
        }
        return 0;
    }
    int handout(uint64_t off, uint8_t *out, uint64_t n)
    {
        CHECK(off + n <= staging.size(), "hand-out [%llu, +%llu) of %zu", (unsigned long long)off, (unsigned long long)n, staging.size());
        memcpy(out, staging.data() + off, n);
        return 0;
    }
};

static bool same_what(const char *a, const char *b) { return (!a && !b) || (a && b && strcmp(a, b) == 0); }

struct Totals {
    uint64_t runs = 0, tail_moves = 0, window_grows = 0, staging_grows = 0, blocks_redone = 0, footer_waits = 0, straddles = 0, passes = 0;
} totals;

// One run: the input in the given chunks (the last one with eof), every feed with `cap` bytes of room.
static void run(const World &w, const Verdict &want, const std::vector<uint64_t> &cuts, uint64_t window, uint64_t staging, uint64_t cap, uint32_t batch,
                const char *label)
{
    FakeDev dev;
    BzsStream<FakeDev> walk;
    dev.w = &w;
    dev.walk = &walk;
    dev.batch = batch;
    CHECK(walk.begin(&dev, w.ctx_level, window, staging) == 0, "begin");
    const uint64_t N = w.in.size();
    std::vector<uint8_t> got, obuf(cap);
    std::vector<uint8_t> chunk;
    int rc = 0;
    bool done = false;
    uint64_t at = 0;
    for (size_t c = 0; c <= cuts.size() && rc == 0 && !done; c++) {
        const uint64_t hi = c < cuts.size() ? cuts[c] : N;
        const bool eof = c == cuts.size();
        chunk.assign(w.in.begin() + (ptrdiff_t)at, w.in.begin() + (ptrdiff_t)hi); // (its own allocation: a read past the feed is seen)
        uint64_t off = 0;
        for (uint64_t guard = 0;; guard++) {
            CHECK(guard < 100000, "%s: the feed loop does not end", label);
            uint64_t used = 0, outn = 0;
            bool fin = false;
            const bool pending = walk.s_off < walk.s_len;
            rc = walk.feed(chunk.data() + off, chunk.size() - off, eof, &used, obuf.data(), cap, &outn, &fin);
            CHECK(used <= chunk.size() - off && outn <= cap, "%s: used %llu of %llu, wrote %llu of %llu", label, (unsigned long long)used,
                  (unsigned long long)(chunk.size() - off), (unsigned long long)outn, (unsigned long long)cap);
            got.insert(got.end(), obuf.begin(), obuf.begin() + (ptrdiff_t)outn);
            if (rc != 0) break;
            CHECK(!((chunk.size() - off > 0 || pending) && !used && !outn && !fin), "%s: a feed that did nothing", label);
            off += used;
            done = fin;
            if (done) break;
            if (off == chunk.size() && outn < cap && !eof) break;
        }
        at = hi;
    }
    totals.runs++;
    totals.passes += walk.st.passes;
    totals.tail_moves += walk.st.tail_moves;
    totals.window_grows += walk.st.window_grows;
    totals.staging_grows += walk.st.staging_grows;
    totals.blocks_redone += walk.st.blocks_redone;
    totals.footer_waits += walk.st.footer_waits;
    totals.straddles += walk.st.straddles;
    CHECK(rc == want.status, "%s: status %d, the whole input judged at once: %d (kind %u at bit %llu)", label, rc, want.status, want.err.kind,
          (unsigned long long)want.err.bit);
    CHECK(walk.consumed == want.consumed, "%s: consumed %llu, want %llu", label, (unsigned long long)walk.consumed, (unsigned long long)want.consumed);
    if (rc == 0) {
        CHECK(done, "%s: not done", label);
        CHECK(got == want.out, "%s: %zu bytes of output, want %zu (or other bytes)", label, got.size(), want.out.size());
        CHECK(walk.st.out_bytes == got.size() && walk.total_out == got.size(), "%s: out_bytes", label);
        CHECK(walk.st.window_peak <= std::max<uint64_t>(window, 8 + 80) + N, "%s: window_peak", label);
        uint64_t used = 0, outn = 0;
        bool fin = false;
        uint8_t more[3] = {1, 2, 3};
        CHECK(walk.feed(more, 3, false, &used, obuf.data(), cap, &outn, &fin) == 0 && used == 3 && outn == 0 && fin, "%s: a feed behind done", label);
    } else {
        const BzsError &e = walk.err, &x = want.err;
        CHECK(e.kind == x.kind && e.bit == x.bit && e.stream == x.stream && e.block == x.block && e.level == x.level && same_what(e.what, x.what),
              "%s: names kind %u, stream %zu, block %zu, bit %llu (%s); want kind %u, stream %zu, block %zu, bit %llu (%s)", label, e.kind, e.stream,
              e.block, (unsigned long long)e.bit, e.what ? e.what : "-", x.kind, x.stream, x.block, (unsigned long long)x.bit, x.what ? x.what : "-");
        CHECK(got.size() <= want.out.size() && std::equal(got.begin(), got.end(), want.out.begin()), "%s: the bytes handed out are no prefix", label);
        uint64_t used = 0, outn = 0;
        bool fin = false;
        CHECK(walk.feed(nullptr, 0, true, &used, obuf.data(), cap, &outn, &fin) == BZS_E_STATE, "%s: a feed behind an error", label);
    }
}

int main(int argc, char **argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: dstream_host <seed> <cases>\n");
        return 2;
    }
    rng_state = strtoull(argv[1], nullptr, 10) * 0x9E3779B97F4A7C15ull + 1;
    const int cases = atoi(argv[2]);
    const uint64_t windows[] = {16, 64, 200, 100000}, stagings[] = {1, 50, 100000}, caps[] = {1, 7, 1u << 20};
    const uint32_t batches[] = {1, 2, 3, 1000};
    static_assert(BZS_BLOCK_BYTES_MAX > 4000000 && BZS_BLOCK_BYTES_MAX < 4300000, "the bound of one block");
    for (int t = 0; t < cases; t++) {
        const int dmg = t < 2 * D_COUNT ? t % D_COUNT : (below(3) ? (int)below(D_COUNT) : D_NONE);
        const World w = make_world(dmg);
        const Verdict want = judge(w);
        const uint64_t N = w.in.size();
        char label[160];
        // byte at a time and in one piece: every room, every cap
        for (uint64_t win : windows)
            for (uint64_t stg : stagings)
                for (uint64_t cap : caps) {
                    const uint32_t batch = batches[below(4)];
                    std::vector<uint64_t> each;
                    for (uint64_t k = 1; k < N; k++) each.push_back(k);
                    snprintf(label, sizeof label, "case %d (damage %d), byte by byte, window %llu, staging %llu, cap %llu, batch %u", t, dmg,
                             (unsigned long long)win, (unsigned long long)stg, (unsigned long long)cap, batch);
                    run(w, want, each, win, stg, cap, batch, label);
                    snprintf(label, sizeof label, "case %d (damage %d), one piece, window %llu, staging %llu, cap %llu, batch %u", t, dmg,
                             (unsigned long long)win, (unsigned long long)stg, (unsigned long long)cap, batch);
                    run(w, want, {}, win, stg, cap, batch, label);
                }
        // every two-chunk split, the rooms and caps taking turns
        for (uint64_t k = 0; k <= N; k++) {
            const uint64_t win = windows[(k + (uint64_t)t) % 4], stg = stagings[(k / 4) % 3], cap = caps[(k / 12) % 3];
            const uint32_t batch = batches[(k / 3) % 4];
            snprintf(label, sizeof label, "case %d (damage %d), split at %llu, window %llu, staging %llu, cap %llu, batch %u", t, dmg,
                     (unsigned long long)k, (unsigned long long)win, (unsigned long long)stg, (unsigned long long)cap, batch);
            run(w, want, {k}, win, stg, cap, batch, label);
        }
    }
    // a run that reached none of a kind is a failure, not a pass
    CHECK(totals.tail_moves > 0, "no tail was moved");
    CHECK(totals.window_grows > 0, "no window grew");
    CHECK(totals.staging_grows > 0, "no staging buffer grew");
    CHECK(totals.blocks_redone > 0, "no block was redone");
    CHECK(totals.footer_waits > 0, "no footer waited for what follows it");
    CHECK(totals.straddles > 0, "no magic straddled two scans");
    printf("%d cases held (%llu runs, %llu passes; %llu tail moves, %llu window grows, %llu staging grows, %llu blocks redone, %llu footer waits, "
           "%llu magics across a feed)\n",
           cases, (unsigned long long)totals.runs, (unsigned long long)totals.passes, (unsigned long long)totals.tail_moves,
           (unsigned long long)totals.window_grows, (unsigned long long)totals.staging_grows, (unsigned long long)totals.blocks_redone,
           (unsigned long long)totals.footer_waits, (unsigned long long)totals.straddles);
    return 0;
}
