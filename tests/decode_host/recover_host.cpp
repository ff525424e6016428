// recover_host.cpp -- the walk of bzh_recover (banzai_amd/csrc/decode_recover_plan.h) against a restatement that makes ONE pass over
// all candidates and knows no batches, built with g++ -fsanitize=address,undefined.  The world is made up: a buffer is a list of
// magics with what the entropy stage would report at each, and what the back of the decoder would find for each block (size, CRC,
// an end in four equal bytes).  The walk is run over it in batches of 1, 2, 3, 4, 5, 7, 8, 16 and 1000 candidates, so that a batch
// edge falls at every position -- between a stream's last block and its footer in particular.  The restatement decides
// STREAM_OK by walking back over its entries when a footer arrives; the walk under test carries a running fold.
//
//   recover_host <seed> <cases>     exit status 0: every case held for every batch size (and the fixed ones)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../banzai_amd/csrc/decode_recover_plan.h"

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
            fprintf(stderr, "recover_host: %s: ", #cond);     \
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
    uint32_t got_crc; // back_emit, the empty window
};
enum Damage { D_NONE, D_KIND, D_BLOCK_CRC, D_BAD_END, D_OVER_CTX, D_OVER_CTX_KERNEL, D_OVER_STREAM, D_NO_MAGIC, D_COUNT };
enum FooterDamage { F_NONE, F_LOST, F_TRUNC, F_CRC, F_COUNT };
struct World {
    std::vector<Cand> cands;
    uint8_t head[4] = {0, 0, 0, 0};
    uint64_t n = 0;
    int ctx_level = 5;
};
struct Opts {
    int streams = -1;     // -1: 0..4
    int damage = -1;      // -1: mixed; else every hit block is damaged this way
    int hit = -1;         // -1: random blocks; else the block of this position in every stream (a stream of fewer: its last)
    int fdamage = -1;     // footer damage of every stream; -1: mixed
    bool all_lost = false, lose_header = false, planted = false;
};

static Cand clean_block(uint64_t pos, uint64_t span, uint32_t nblock_max)
{
    Cand c{};
    c.pos = pos;
    c.r.kind = BZD_OK;
    c.r.crc = c.got_crc = (uint32_t)rnd();
    c.r.nblock = 1 + (uint32_t)below(nblock_max);
    c.r.end_bit = pos + span;
    c.size = 1 + below(5000);
    return c;
}

static void damage_block(Cand &c, int dmg, const World &w, uint32_t lv)
{
    switch (dmg) {
    case D_KIND: {
        const uint32_t kinds[] = {BZD_K_TRUNC, BZD_K_FORMAT, BZD_K_RANDOMISED};
        c.r.kind = kinds[below(3)];
        c.r.errpos = c.pos + 48 + below(c.r.end_bit - c.pos - 48);
        c.r.end_bit = 0;
        break;
    }
    case D_BLOCK_CRC: c.got_crc ^= 1u << below(32); break;
    case D_BAD_END: c.bad_end = true; break;
    case D_OVER_CTX: c.r.nblock = 100000u * (uint32_t)w.ctx_level + 1 + (uint32_t)below(1000); break; // (the walk's own check)
    case D_OVER_CTX_KERNEL:                                                                            // (what the kernel says of it)
        c.r.kind = BZD_K_FORMAT;
        c.r.errpos = c.pos + 60;
        c.r.end_bit = 0;
        break;
    case D_OVER_STREAM: // above its stream's level, within the context's: kept, its stream not STREAM_OK
        if ((int)lv < w.ctx_level) c.r.nblock = 100000u * lv + 1 + (uint32_t)below(100000u * ((uint32_t)w.ctx_level - lv));
        break;
    default: break;
    }
}

static World make_world(const Opts &o)
{
    World w;
    w.ctx_level = 1 + (int)below(9);
    const uint32_t nstreams = o.streams >= 0 ? (uint32_t)o.streams : (uint32_t)below(5);
    uint64_t bit = 0;
    bool header_here = true; // a stream header stands at `bit`
    std::vector<uint32_t> levels(nstreams + 1);
    for (uint32_t q = 0; q <= nstreams; q++) levels[q] = 1 + (uint32_t)below(9);
    if (nstreams) {
        memcpy(w.head, "BZh", 3);
        w.head[3] = (uint8_t)('0' + levels[0]);
        if (o.lose_header || below(8) == 0) {
            memset(w.head, 0, 4);
            header_here = false;
        }
    } else if (below(2)) {
        memcpy(w.head, "junk", 4);
    }
    size_t pending_footer = SIZE_MAX; // the footer whose `follow` waits for the next stream's header
    for (uint32_t q = 0; q < nstreams; q++) {
        const uint32_t lv = levels[q];
        if (pending_footer != SIZE_MAX) {
            w.cands[pending_footer].r.follow = header_here ? (0x100u | lv) : 2u;
            pending_footer = SIZE_MAX;
        }
        bit += 32;
        const uint32_t nb = (uint32_t)below(5);
        const uint32_t nmax = 100000u * (uint32_t)std::min<int>((int)lv, w.ctx_level);
        uint32_t fold = 0;
        for (uint32_t b = 0; b < nb; b++) {
            const uint64_t span = 90 + below(400);
            Cand c = clean_block(bit, span, nmax);
            const bool hit = o.all_lost || (o.hit >= 0 ? (b == (uint32_t)std::min<int>(o.hit, (int)nb - 1)) : below(4) == 0);
            int dmg = D_NONE;
            if (hit) dmg = o.all_lost ? 1 + (int)below(D_OVER_CTX_KERNEL) : o.damage >= 0 ? o.damage : (int)below(D_COUNT);
            if (o.all_lost && dmg == D_OVER_CTX && w.ctx_level == 9) dmg = D_BLOCK_CRC;
            if (dmg == D_OVER_CTX && w.ctx_level == 9) dmg = D_OVER_CTX_KERNEL; // (900001 bytes: the format has no such block, the kernel refuses it)
            damage_block(c, dmg, w, lv);
            fold = ((fold << 1) | (fold >> 31)) ^ c.r.crc;
            const bool outer_lost = c.r.kind != BZD_OK || c.bad_end || c.got_crc != c.r.crc || c.r.nblock > 100000u * (uint32_t)w.ctx_level;
            for (uint32_t x = (uint32_t)below(3) + (o.planted ? 1 : 0); x > 0; x--) { // magics inside the payload: anything may be reported there
                Cand in{};
                in.pos = bit + 49 + below(span - 50);
                in.footer = below(3) == 0;
                if (in.footer) {
                    in.r.kind = below(2) ? BZD_OK : BZD_K_TRUNC;
                    in.r.crc = below(2) ? 0 : (uint32_t)rnd();
                    in.r.end_bit = (in.pos + 80 + 7) / 8 * 8;
                    in.r.follow = below(2) ? (0x100u | (1 + (uint32_t)below(9))) : 2u;
                } else if (!o.all_lost && ((o.planted && outer_lost) || below(2))) { // a block that verifies: kept where the outer one is lost
                    in = clean_block(in.pos, 81 + below(200), 100000u * (uint32_t)w.ctx_level);
                    if (below(4) == 0) in.got_crc ^= 4;
                } else {
                    in.r.kind = below(2) ? BZD_K_FORMAT : BZD_K_TRUNC;
                    in.r.errpos = in.pos + 50 + below(1000);
                    in.r.crc = (uint32_t)rnd();
                }
                w.cands.push_back(in);
            }
            bit += span;
            if (dmg != D_NO_MAGIC) w.cands.push_back(c);
        }
        Cand f{};
        f.pos = bit;
        f.footer = true;
        f.r.kind = BZD_OK;
        f.r.crc = fold;
        const int fd = o.fdamage >= 0 ? o.fdamage : below(3) == 0 ? (int)below(F_COUNT) : F_NONE;
        if (fd == F_CRC) f.r.crc ^= 1u << below(32);
        bit = (bit + 80 + 7) / 8 * 8;
        f.r.end_bit = bit;
        if (fd == F_TRUNC) {
            f.r.kind = BZD_K_TRUNC;
            f.r.errpos = bit;
        }
        if (fd != F_LOST) {
            w.cands.push_back(f);
            pending_footer = w.cands.size() - 1;
        }
        header_here = true;
        if (below(3) == 0) { // foreign bytes behind the stream, with a loose footer or a loose block in them now and then
            const uint64_t gap = 8 * (1 + below(40));
            if (gap >= 160 && below(2)) {
                Cand x{};
                x.pos = bit + below(gap - 100);
                x.footer = below(2);
                if (x.footer) {
                    x.r.kind = BZD_OK;
                    x.r.crc = below(2) ? 0 : (uint32_t)rnd();
                    x.r.end_bit = (x.pos + 80 + 7) / 8 * 8;
                    x.r.follow = below(2) ? (0x100u | (1 + (uint32_t)below(9))) : 2u;
                } else {
                    x = clean_block(x.pos, 81 + below(300), 100000u * (uint32_t)w.ctx_level);
                }
                w.cands.push_back(x);
            }
            bit += gap;
            header_here = below(2); // (a header behind foreign bytes: only a loose footer can report it)
            if (pending_footer != SIZE_MAX) {
                w.cands[pending_footer].r.follow = 2u;
                pending_footer = SIZE_MAX;
            }
        } else if (below(6) == 0) {
            header_here = false; // the next stream's header is lost
        }
    }
    if (pending_footer != SIZE_MAX) w.cands[pending_footer].r.follow = 0;
    w.n = (bit + 7) / 8 + below(3);
    std::sort(w.cands.begin(), w.cands.end(), [](const Cand &a, const Cand &b) { return a.pos < b.pos; });
    // one magic a bit position, as the scan reports them
    w.cands.erase(std::unique(w.cands.begin(), w.cands.end(), [](const Cand &a, const Cand &b) { return a.pos == b.pos; }), w.cands.end());
    return w;
}

// ---- the restatement: one pass, rules 1 to 5 of include/bzhip.h ----------------------------------------------------------
struct Told {
    std::vector<bzh_recover_entry> ent;
    bzh_recover_stats st{};
    uint64_t total = 0;
};
static Told restate(const World &w)
{
    Told t;
    std::vector<std::pair<uint64_t, uint32_t>> hdr; // accepted headers: bit, level
    std::vector<int> via_header;                    // per entry: the level of the header it starts behind, 0: none
    std::vector<uint32_t> nblock;                   // per entry
    if (w.n >= 4 && !memcmp(w.head, "BZh", 3) && w.head[3] >= '1' && w.head[3] <= '9') hdr.push_back({0, (uint32_t)(w.head[3] - '0')});
    auto header_at = [&](uint64_t bitpos) -> uint32_t {
        uint32_t lv = 0;
        for (auto &h : hdr)
            if (h.first == bitpos) lv = h.second; // (the latest report of it)
        return lv;
    };
    uint64_t shadow = 0;
    for (const Cand &c : w.cands) {
        if (!c.footer) t.st.candidates++;
        if (c.pos < shadow) {
            t.st.shadowed++;
            continue;
        }
        if (c.footer) {
            t.st.footers++;
            const bool intact = c.r.kind == BZD_OK;
            if (!t.ent.empty() && t.ent.back().kind == 0 && t.ent.back().end_bit == c.pos) {
                t.ent.back().flags |= BZH_REC_STREAM_END;
                // back over the run
                size_t i = t.ent.size() - 1;
                bool reaches = false;
                for (;;) {
                    if (t.ent[i].kind != 0 || !(t.ent[i].flags & BZH_REC_JOINED)) break;
                    if (via_header[i]) {
                        reaches = true;
                        break;
                    }
                    if (i == 0) break;
                    i--;
                }
                if (reaches && intact) {
                    const uint32_t lv = (uint32_t)via_header[i];
                    uint32_t fold = 0;
                    bool fits = true;
                    for (size_t j = i; j < t.ent.size(); j++) {
                        fold = ((fold << 1) | (fold >> 31)) ^ t.ent[j].crc;
                        fits = fits && nblock[j] <= 100000u * lv;
                    }
                    if (fits && fold == c.r.crc) {
                        t.ent.back().flags |= BZH_REC_STREAM_OK;
                        t.st.streams_ok++;
                    }
                }
            } else if (intact && c.r.crc == 0 && c.pos >= 32 && header_at(c.pos - 32)) {
                t.st.streams_ok++;
            }
            if (intact && (c.r.follow & 0x100u)) hdr.push_back({c.r.end_bit, c.r.follow & 15u});
            continue;
        }
        bzh_recover_entry e{};
        e.bit_pos = c.pos;
        e.out_off = t.total;
        e.crc = c.pos + 80 <= 8 * w.n ? c.r.crc : 0;
        uint32_t kind = 0;
        uint64_t err = c.pos;
        if (c.r.kind != BZD_OK)
            kind = c.r.kind, err = c.r.errpos;
        else if (c.r.nblock > 100000u * (uint32_t)w.ctx_level)
            kind = BZH_LOST_FORMAT;
        else if (c.bad_end)
            kind = BZH_LOST_FORMAT;
        else if (c.got_crc != c.r.crc)
            kind = BZH_LOST_BLOCK_CRC;
        int via = 0;
        if (kind == 0) {
            e.end_bit = c.r.end_bit;
            e.out_len = (uint32_t)c.size;
            via = c.pos >= 32 ? (int)header_at(c.pos - 32) : 0;
            if (via || (!t.ent.empty() && t.ent.back().kind == 0 && t.ent.back().end_bit == c.pos)) e.flags |= BZH_REC_JOINED;
            t.total += c.size;
            shadow = c.r.end_bit;
            t.st.kept++;
        } else {
            e.kind = kind;
            e.err_bit = err;
            t.st.lost++;
        }
        t.ent.push_back(e);
        via_header.push_back(via);
        nblock.push_back(c.r.nblock);
    }
    t.st.out_bytes = t.total;
    return t;
}

static void run_case(const World &w, const Told &t, uint32_t max_batch, uint64_t cap)
{
    std::vector<uint64_t> cl;
    for (const Cand &c : w.cands) cl.push_back(c.pos << 1 | (c.footer ? 1 : 0));
    BzrWalk walk;
    walk.cands = cl.data();
    walk.nc = cl.size();
    walk.n = w.n;
    memcpy(walk.head, w.head, 4);
    walk.ctx_level = w.ctx_level;
    walk.start();
    size_t first, given = 0, batches = 0, kept_items = 0;
    uint32_t B;
    while (walk.next_batch(max_batch, &first, &B)) {
        CHECK(B >= 1 && B <= max_batch && first + B <= cl.size() && first >= given, "batch [%zu, +%u) of %zu", first, B, cl.size());
        given = first + B;
        std::vector<BzdResult> res(B); // exactly the batch: one slot further is a report
        for (uint32_t q = 0; q < B; q++) res[q] = w.cands[first + q].r;
        walk.feed(res.data());
        uint32_t last_slot = 0;
        for (BzrItem &it : walk.items) {
            CHECK(it.slot < B && (it.slot > last_slot || &it == &walk.items[0]), "slot %u of %u", it.slot, B);
            last_slot = it.slot;
            const Cand &c = w.cands[first + it.slot];
            CHECK(!c.footer && c.r.kind == BZD_OK && it.nblock == c.r.nblock, "item at slot %u is no clean block", it.slot);
            it.size = c.size;
            it.bad_end = c.bad_end;
            it.got_crc = c.bad_end ? 0xDEADBEEFu : c.got_crc; // (no CRC is taken of a block with an open run)
        }
        const size_t before = walk.entries.size();
        const bool over_before = walk.over;
        walk.select();
        walk.place(cap);
        CHECK(walk.over == (over_before || walk.total_out > cap), "over %d at a total of %llu, cap %llu", (int)walk.over,
              (unsigned long long)walk.total_out, (unsigned long long)cap);
        for (const BzrItem &it : walk.items) {
            if (!it.kept) continue;
            kept_items++;
            bool found = false;
            for (size_t i = before; i < walk.entries.size(); i++) {
                const bzh_recover_entry &e = walk.entries[i];
                if (e.bit_pos == w.cands[first + it.slot].pos) found = e.kind == 0 && e.out_off == it.base && e.out_len == it.size;
            }
            CHECK(found, "a kept item at slot %u without its entry", it.slot);
        }
        batches++;
        CHECK(batches <= cl.size() + 1, "the walk does not end");
    }
    walk.finish();
    CHECK(walk.entries.size() == t.ent.size(), "%zu entries, the restatement %zu (batch %u)", walk.entries.size(), t.ent.size(), max_batch);
    CHECK(walk.runs.size() == walk.entries.size(), "runs");
    for (size_t i = 0; i < t.ent.size(); i++) {
        const bzh_recover_entry &a = walk.entries[i], &b = t.ent[i];
        CHECK(!memcmp(&a, &b, sizeof a),
              "entry %zu (batch %u): bit %llu end %llu off %llu len %u crc %08x kind %u flags %u err %llu, the restatement bit %llu end %llu off %llu len %u "
              "crc %08x kind %u flags %u err %llu",
              i, max_batch, (unsigned long long)a.bit_pos, (unsigned long long)a.end_bit, (unsigned long long)a.out_off, a.out_len, a.crc, a.kind,
              a.flags, (unsigned long long)a.err_bit, (unsigned long long)b.bit_pos, (unsigned long long)b.end_bit, (unsigned long long)b.out_off,
              b.out_len, b.crc, b.kind, b.flags, (unsigned long long)b.err_bit);
    }
    const bzh_recover_stats &s = walk.stats;
    CHECK(s.candidates == t.st.candidates && s.kept == t.st.kept && s.lost == t.st.lost && s.shadowed == t.st.shadowed && s.footers == t.st.footers &&
              s.streams_ok == t.st.streams_ok && s.out_bytes == t.st.out_bytes,
          "stats (batch %u): kept %llu/%llu lost %llu/%llu shadowed %llu/%llu footers %llu/%llu streams_ok %llu/%llu", max_batch,
          (unsigned long long)s.kept, (unsigned long long)t.st.kept, (unsigned long long)s.lost, (unsigned long long)t.st.lost,
          (unsigned long long)s.shadowed, (unsigned long long)t.st.shadowed, (unsigned long long)s.footers, (unsigned long long)t.st.footers,
          (unsigned long long)s.streams_ok, (unsigned long long)t.st.streams_ok);
    CHECK(s.batches == batches && kept_items == t.st.kept, "batches %llu, kept items %zu", (unsigned long long)s.batches, kept_items);
    CHECK(s.kept + s.lost + s.shadowed + s.footers == cl.size(), "every magic is kept, lost, shadowed or a footer outside the kept blocks");
    CHECK(walk.total_out == t.total && walk.over == (t.total > cap), "total %llu / %llu, over %d", (unsigned long long)walk.total_out,
          (unsigned long long)t.total, (int)walk.over);
}

static void run_world(const World &w)
{
    const Told t = restate(w);
    // the report as a whole: bzr_report_check takes what the walk wrote, and `max` too small is a count the caller compares
    size_t bad = 0, kept = 0;
    uint64_t body = 0;
    // (made-up ends may lie behind the made-up input: the check is given room)
    CHECK(bzr_report_check(t.ent.data(), t.ent.size(), UINT64_MAX / 8, &bad, &body, &kept) == nullptr && kept == t.st.kept, "the report of the walk is refused at %zu", bad);
    for (uint32_t mb : {1u, 2u, 3u, 4u, 5u, 7u, 8u, 16u, 1000u}) {
        run_case(w, t, mb, UINT64_MAX);
        run_case(w, t, mb, t.total);
        if (t.total) run_case(w, t, mb, t.total - 1);
        run_case(w, t, mb, 0);
    }
}

int main(int argc, char **argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: recover_host <seed> <cases>\n");
        return 2;
    }
    rng_state = strtoull(argv[1], nullptr, 10) * 0x9E3779B97F4A7C15ull + 1;
    const size_t cases = strtoull(argv[2], nullptr, 10);
    static_assert(sizeof(bzh_recover_entry) == 48, "the entry has no padding: entries are compared as bytes");
    for (int rep = 0; rep < 10; rep++) {
        for (int d = 0; d < D_COUNT; d++)      // each loss kind in every position, every footer damage beside it
            for (int hit = 0; hit < 4; hit++)
                for (int fd = 0; fd < F_COUNT; fd++) {
                    Opts o;
                    o.damage = d, o.hit = hit, o.fdamage = fd;
                    o.streams = 1 + (int)below(4);
                    run_world(make_world(o));
                }
        Opts o;
        o.all_lost = true;
        run_world(make_world(o)); // everything lost
        o = Opts{};
        o.streams = 0;
        run_world(make_world(o)); // nothing at all
        o = Opts{};
        o.lose_header = true;
        run_world(make_world(o)); // the first stream header lost
        o = Opts{};
        o.planted = true, o.damage = D_KIND, o.hit = rep % 4;
        run_world(make_world(o)); // a kept block planted inside a lost one
    }
    for (size_t c = 0; c < cases; c++) run_world(make_world(Opts{}));
    printf("recover_host: %zu cases held for every batch size\n", cases);
    return 0;
}
