// layout_host.cpp -- how the library cuts its workspaces (banzai_amd/csrc/batch.h: the carver, layout_batch and the views of
// borrowed arrays; decode_plan.h: the decoder's tables; encode_plan.h: the plan's two workspaces), built with
// g++ -fsanitize=address,undefined.  The library calls the same text; there an array that overlaps its neighbour or a view that
// outgrows its lender is a kernel writing over another kernel's data, here it is a failed comparison or a sanitizer report.
//
//   layout_host      exit status 0: every check held
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>

#include <algorithm>
#include <vector>

#include "../../banzai_amd/csrc/decode_plan.h"
#include "../../banzai_amd/csrc/encode_plan.h"

#define CHECK(cond, ...)                                      \
    do {                                                      \
        if (!(cond)) {                                        \
            fprintf(stderr, "layout_host: %s: ", #cond);      \
            fprintf(stderr, __VA_ARGS__);                     \
            fprintf(stderr, "\n");                            \
            exit(1);                                          \
        }                                                     \
    } while (0)

// Room for a real pass.  Up to 64 MiB it is a heap allocation of exactly the measured size, and the first and last byte of every
// array are written: AddressSanitizer sees an array that leaves it.  Beyond that (32.4 GB at level 9 and 576 blocks) it is
// address space without memory behind it: real addresses, never touched.
struct Room {
    uint8_t *p = nullptr;
    size_t bytes = 0;
    bool heap = false;
    explicit Room(size_t n) : bytes(n), heap(n <= ((size_t)64 << 20))
    {
        if (heap) {
            p = (uint8_t *)aligned_alloc(256, n); // (n is a multiple of 256: the carver's total)
        } else {
            void *m = mmap(nullptr, n, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
            p = m == MAP_FAILED ? nullptr : (uint8_t *)m;
        }
        CHECK(p != nullptr, "no room of %zu bytes", n);
    }
    ~Room()
    {
        if (heap) free(p);
        else munmap(p, bytes);
    }
};

// What every layout owes: a measuring pass and a real pass take the same arrays at the same offsets and come to the same total;
// every array starts at a multiple of 256 bytes from a 256-byte aligned base, lies inside [base, base + total) and ends at or
// before the next one begins (the takes ascend, so that is "overlaps no other").
static void check_spans(const char *what, const std::vector<CarveSpan> &measured, size_t measured_bytes, const std::vector<CarveSpan> &real,
                        size_t real_bytes, const Room &room)
{
    CHECK(measured_bytes == real_bytes && real_bytes == room.bytes, "%s: measured %zu bytes, carved %zu, room %zu", what, measured_bytes, real_bytes, room.bytes);
    CHECK(measured.size() == real.size() && !real.empty(), "%s: %zu takes measured, %zu carved", what, measured.size(), real.size());
    CHECK(((uintptr_t)room.p & 255u) == 0, "%s: base not aligned", what);
    for (size_t k = 0; k < real.size(); k++) {
        const CarveSpan &m = measured[k], &r = real[k];
        CHECK(m.off == r.off && m.count == r.count && m.elem == r.elem, "%s: take %zu measured at %zu (%zu x %zu), carved at %zu (%zu x %zu)", what, k,
              m.off, m.count, m.elem, r.off, r.count, r.elem);
        const size_t end = r.off + r.count * r.elem;
        CHECK(r.off % 256 == 0, "%s: take %zu at offset %zu", what, k, r.off);
        CHECK(end <= real_bytes, "%s: take %zu ends at %zu of %zu", what, k, end, real_bytes);
        CHECK(end <= (k + 1 < real.size() ? real[k + 1].off : real_bytes), "%s: take %zu ends at %zu, the next begins at %zu", what, k, end,
              k + 1 < real.size() ? real[k + 1].off : real_bytes);
        if (room.heap && r.count) {
            room.p[r.off] = 1;
            room.p[end - 1] = 1;
        }
    }
}

static size_t span_bytes_at(const std::vector<CarveSpan> &log, const Room &room, const void *array, const char *name)
{
    for (const CarveSpan &s : log)
        if (room.p + s.off == (const uint8_t *)array) return s.count * s.elem;
    CHECK(false, "%s is no array of the layout", name);
    return 0;
}

// ---- layout_batch and its views ---------------------------------------------------------------------------------------
static void batch_case(uint32_t level, uint32_t B)
{
    const uint32_t M = 100000u * level - 1u;
    char what[64];
    snprintf(what, sizeof what, "batch level %u B %u", level, B);
    Batch probe{}, bt{};
    std::vector<CarveSpan> lm, lr;
    const char *misfit = "unset";
    const size_t need = layout_batch(probe, nullptr, B, M, &misfit, &lm);
    CHECK(misfit == nullptr, "%s: %s does not fit", what, misfit);
    CHECK(probe.rle == nullptr && probe.fx_hdr == nullptr && probe.st_mode == nullptr && probe.stat_A == nullptr && probe.nlist == nullptr,
          "%s: a measuring pass formed a pointer", what);
    Room room(need);
    const size_t got = layout_batch(bt, room.p, B, M, nullptr, &lr);
    check_spans(what, lm, need, lr, got, room);
    CHECK(bt.B == B && bt.M == M && bt.S % SORT_TILE == 0 && bt.S > M && bt.S - M <= (uint32_t)SORT_TILE && bt.TPB == bt.S / SORT_TILE, "%s: geometry", what);
    // the round state: RS_ROWS rows of B words, the list lengths, the 64-bit counter -- inside their one take, the counter aligned
    const size_t rs = span_bytes_at(lr, room, bt.st_mode, "st_mode");
    CHECK((uint8_t *)(bt.stat_A + 1) <= (uint8_t *)bt.st_mode + rs && ((uintptr_t)bt.stat_A & 7u) == 0, "%s: the round counter", what);
    CHECK(bt.nlist == bt.st_mode + (size_t)RS_ROWS * B && (uint8_t *)(bt.nlist + 8) <= (uint8_t *)bt.stat_A, "%s: nlist", what);
    CHECK(bt.st_tdst == bt.st_mode + (size_t)(RS_ROWS - 1) * B && bt.actQ + 2 * (size_t)B == bt.c_nolist, "%s: the row table", what);
    // the views: what the table says each lender has is what the carver gave it, and every borrower fits -- worked out here
    // from the kernels' indexing, at both MTF tile sizes, not copied from the table
    BatchView v[BATCH_VIEWS];
    batch_views(B, bt.S, bt.TPB, v);
    const size_t S = bt.S, TPB = bt.TPB, NB = B;
    const size_t list = span_bytes_at(lr, room, bt.listA, "listA");
    for (const uint2 *l : {bt.listB, bt.listC, bt.listD, bt.binned}) CHECK(span_bytes_at(lr, room, l, "list") == list, "%s: the lists differ in size", what);
    const size_t hist = span_bytes_at(lr, room, bt.hist, "hist"), flg = span_bytes_at(lr, room, bt.flg, "flg"), tagg = span_bytes_at(lr, room, bt.tagg, "tagg");
    struct Want {
        const void *view, *lender;
        size_t have, need;
    };
    size_t tlast = 0, tiles = 0;
    for (uint32_t TL : {MTF_TILE, 2u * MTF_TILE}) {
        const size_t MT = (S + TL - 1) / TL;
        tlast = std::max(tlast, NB * MT * 256 * sizeof(int32_t));
        tiles = std::max(tiles, NB * MT * sizeof(MtfTile));
    }
    CHECK(mtf_tile_bytes(B) == (B >= 64 ? 2u * MTF_TILE : MTF_TILE), "%s: tile rule", what);
    const Want want[BATCH_VIEWS] = {
        {list_words(bt.listA), bt.listA, list, NB * S * 8},
        {mtf_tlast(bt), bt.listA, list, tlast},
        {mtf_tiles(bt), bt.listB, list, tiles},
        {huff_ranges(bt), bt.tagg, tagg, NB * 8 * 4},                              // B rows of 8 words
        {refine_carry(bt), bt.tagg, tagg, ((NB - 1) * TPB * 2 + 1 + (TPB - 1) * 2 + 1) * 8}, // word b * TPB * 2 + 1 + tile * 2 is the last one
        {sort_look(bt), bt.hist, hist, NB * TPB * 256 * 8},                        // 256 status words a tile
        {init_digits(bt), bt.flg, flg, ((NB - 1) * (S / 4) + (TPB - 1) * 512 + 384) * 4}, // row (b, tile) at b * S / 4 + tile * 512, 384 words
        {sweep_clist(bt), bt.listD, list, NB * 2 * S * 4},
    };
    for (int k = 0; k < BATCH_VIEWS; k++) {
        CHECK(want[k].view == want[k].lender, "%s: view %s does not start at its lender", what, v[k].name);
        CHECK(v[k].have == want[k].have, "%s: view %s: the table says its lender has %zu bytes, the carver gave %zu", what, v[k].name, v[k].have, want[k].have);
        CHECK(v[k].need >= want[k].need, "%s: view %s: the table asks for %zu bytes, the kernels touch %zu", what, v[k].name, v[k].need, want[k].need);
        CHECK(v[k].need <= v[k].have, "%s: view %s needs %zu bytes of %zu", what, v[k].name, v[k].need, v[k].have);
    }
}

// The two lanes of a context of max_batch blocks: half-batch layouts at arena + k * half, the arena being what ensure_lanes asks
// ensure_arena for (the layout of arena_batch(max_batch) blocks, and at least two halves).
static void lanes_case(uint32_t level, uint32_t max_batch)
{
    const uint32_t M = 100000u * level - 1u, lane_mb = std::max<uint32_t>(1, max_batch / 2);
    Batch probe{}, lane[2] = {};
    const size_t half = layout_batch(probe, nullptr, lane_mb, M);
    const uint32_t want = arena_batch(max_batch, max_batch);
    CHECK(want == max_batch, "lanes max_batch %u: the arena is laid out for %u", max_batch, want);
    const size_t arena = std::max(layout_batch(probe, nullptr, want, M), 2 * half);
    Room room(arena);
    std::vector<CarveSpan> log[2];
    for (int k = 0; k < 2; k++) {
        const size_t got = layout_batch(lane[k], room.p + (size_t)k * half, lane_mb, M, nullptr, &log[k]);
        CHECK(got == half, "lanes level %u max_batch %u: lane %d takes %zu bytes, half is %zu", level, max_batch, k, got, half);
        for (const CarveSpan &s : log[k]) {
            const size_t lo = (size_t)k * half + s.off, hi = lo + s.count * s.elem;
            CHECK(lo >= (size_t)k * half && hi <= (size_t)(k + 1) * half && hi <= arena, "lanes level %u max_batch %u: lane %d reaches [%zu, %zu) of its half / of an arena of %zu",
                  level, max_batch, k, lo, hi, arena);
        }
    }
    CHECK((uint8_t *)lane[1].rle == room.p + half && (uint8_t *)lane[0].fx_hdr < room.p + half, "lanes level %u max_batch %u: the halves meet", level, max_batch);
}

// ---- the decoder's tables ---------------------------------------------------------------------------------------------
static void dec_case(uint32_t level, uint32_t B)
{
    Batch probe{};
    (void)layout_batch(probe, nullptr, 1, 100000u * level - 1u);
    const uint32_t T = probe.S / 4096u; // (UR_TILE, decode.hip)
    DecWs wm{}, wr{};
    std::vector<CarveSpan> lm, lr;
    const size_t need = dec_layout(wm, nullptr, B, T, &lm);
    CHECK(wm.cand == nullptr && wm.small == nullptr, "dec: a measuring pass formed a pointer");
    Room room(need);
    const size_t got = dec_layout(wr, room.p, B, T, &lr);
    char what[64];
    snprintf(what, sizeof what, "dec level %u B %u", level, B);
    check_spans(what, lm, need, lr, got, room);
    CHECK(wr.B == B && wr.T == T && lr.size() == 21, "%s: %zu tables", what, lr.size());
    CHECK(span_bytes_at(lr, room, wr.toff, "toff") == (size_t)B * T * 4 && span_bytes_at(lr, room, wr.res, "res") == (size_t)B * sizeof(BzdResult) &&
              span_bytes_at(lr, room, wr.wbase, "wbase") == (size_t)B * 8 && span_bytes_at(lr, room, wr.scancnt, "scancnt") == 4,
          "%s: table sizes", what);
}

// ---- the plan's workspaces ----------------------------------------------------------------------------------------------
static void plan_case(uint32_t level, uint64_t n, uint32_t extra)
{
    const uint32_t M = 100000u * level - 1u;
    std::vector<CarveSpan> lm, lr;
    const PlanWs wm = plan_layout(nullptr, n, M, extra, &lm);
    CHECK(wm.pa.lrs == nullptr && wm.crcacc == nullptr, "plan: a measuring pass formed a pointer");
    Room room(wm.bytes);
    const PlanWs wr = plan_layout(room.p, n, M, extra, &lr);
    char what[96];
    snprintf(what, sizeof what, "plan level %u n %llu extra %u", level, (unsigned long long)n, extra);
    check_spans(what, lm, wm.bytes, lr, wr.bytes, room);
    const uint64_t ntiles = (n + 4095) / 4096, maxblocks = n / ((uint64_t)(M - 1) * 4 / 5) + 4 + extra;
    CHECK(wr.pa.ntiles == ntiles && wr.pa.ngran == ntiles * 64 && wr.pa.maxblocks == maxblocks && wr.pa.n == n && wr.pa.M == M, "%s: counts", what);
    CHECK(span_bytes_at(lr, room, wr.pa.frs, "frs") >= (ntiles + 1) * 4 && span_bytes_at(lr, room, wr.pa.tc, "tc") >= (ntiles + 1) * 8 &&
              span_bytes_at(lr, room, wr.pa.nrsg, "nrsg") >= (ntiles * 64 + 1) * 4 && span_bytes_at(lr, room, wr.pa.blocks, "blocks") == maxblocks * sizeof(BlockDesc) &&
              span_bytes_at(lr, room, wr.pa.aux, "aux") == maxblocks * sizeof(BlockAux) && span_bytes_at(lr, room, wr.crcacc, "crcacc") == maxblocks * 4,
          "%s: table sizes", what);
    // blocks | aux | nblocks come back in one copy (rle1_plan_split): consecutive, the count behind the records
    CHECK((const uint8_t *)wr.pa.blocks < (const uint8_t *)wr.pa.aux && (const uint8_t *)wr.pa.aux < (const uint8_t *)wr.pa.nblocks &&
              (const uint8_t *)wr.pa.nblocks < (const uint8_t *)wr.crcacc, "%s: blocks, aux, nblocks out of order", what);
}

static void many_case(uint32_t level, const std::vector<size_t> &lens)
{
    const uint32_t M = 100000u * level - 1u, D = (M - 1u) * 4u / 5u;
    std::vector<CarveSpan> lm, lr;
    const ManyWs wm = many_layout(nullptr, lens.data(), lens.size(), M, &lm);
    CHECK(wm.gbuf == nullptr && wm.binp == nullptr, "many: a measuring pass formed a pointer");
    Room room(wm.bytes);
    const ManyWs wr = many_layout(room.p, lens.data(), lens.size(), M, &lr);
    char what[96];
    snprintf(what, sizeof what, "many level %u count %zu", level, lens.size());
    check_spans(what, lm, wm.bytes, lr, wr.bytes, room);
    uint64_t total = 0, slots = 0;
    for (size_t l : lens) {
        total += l;
        if (l) slots += l / D + 1; // an empty input has no block and no slot
        CHECK(many_slots(l, M) == (l ? l / D + 1 : 0), "%s: slots of an input of %zu bytes", what, l);
    }
    CHECK(wr.ng == total + lens.size() && wr.slots == slots && wr.maxblocks == wr.ng / D + 4 + lens.size(), "%s: counts", what);
    CHECK(span_bytes_at(lr, room, wr.gbuf, "gbuf") == wr.ng + 32 && span_bytes_at(lr, room, wr.tab, "tab") == lens.size() * sizeof(ManyInput) &&
              span_bytes_at(lr, room, wr.sb, "sb") == slots * sizeof(BlockDesc) && span_bytes_at(lr, room, wr.sa, "sa") == slots * sizeof(BlockAux) &&
              span_bytes_at(lr, room, wr.binp, "binp") == wr.maxblocks * 4,
          "%s: table sizes", what);
    // the plan over the guarded buffer has room for every block the inputs can be cut into (plan_layout with one extra an input)
    CHECK(plan_layout(nullptr, wr.ng, M, (uint32_t)lens.size()).pa.maxblocks == wr.maxblocks, "%s: the plan's bound", what);
}

int main()
{
    { // the carver alone: a null base measures and forms no pointer (UBSan's pointer-overflow check is on), a real one carves
        Carver c(nullptr);
        CHECK(c.take<uint8_t>(1) == nullptr && c.take<uint64_t>(33) == nullptr && c.take<uint32_t>(0) == nullptr && c.take<uint2>(7) == nullptr, "null base");
        CHECK(c.bytes() == 256 + 512 + 0 + 256, "a null carver measured %zu", c.bytes());
        Room room(c.bytes());
        Carver r(room.p);
        uint8_t *a = r.take<uint8_t>(1);
        uint64_t *b = r.take<uint64_t>(33);
        uint32_t *z = r.take<uint32_t>(0);
        uint2 *d = r.take<uint2>(7);
        CHECK(a == room.p && (uint8_t *)b == room.p + 256 && (uint8_t *)z == room.p + 768 && (uint8_t *)d == room.p + 768 && r.bytes() == c.bytes(), "real base");
        a[0] = 1, b[32] = 1, d[6].y = 1;
    }
    const uint32_t Bs[] = {1, 2, 8, 9, 16, 17, 112, 576};
    for (uint32_t level = 1; level <= 9; level++) {
        for (uint32_t B : Bs) batch_case(level, B);
        for (uint32_t mb : {1u, 2u, 3u, 576u}) lanes_case(level, mb);
        for (uint32_t B : {1u, 576u}) dec_case(level, B);
        for (uint64_t n : {(uint64_t)1, (uint64_t)4095, (uint64_t)4096, (uint64_t)4097, (uint64_t)1 << 20})
            for (uint32_t extra : {0u, 1000u}) plan_case(level, n, extra);
        many_case(level, {5});
        many_case(level, {0, 700001});
        many_case(level, {300000, 0});
        std::vector<size_t> lens(1000);
        for (size_t k = 0; k < lens.size(); k++) lens[k] = k % 7 == 3 ? 0 : (k * 2654435761u) % 5000 + (k % 97 == 0 ? 250000 : 0);
        lens[0] = 0, lens[999] = 0;
        many_case(level, lens);
    }
    // arena_batch: at least 8, then multiples of 16, never beyond max_batch
    for (uint32_t mb : {1u, 2u, 3u, 8u, 9u, 32u, 576u, 1024u})
        for (uint32_t blocks = 0; blocks <= mb + 1; blocks++) {
            const uint32_t w = arena_batch(blocks, mb), b = std::max(1u, std::min(blocks, mb));
            CHECK(w >= b && w <= mb && (w == mb || w == 8 || (w % 16 == 0 && w - b < 16)), "arena_batch(%u, %u) = %u", blocks, mb, w);
        }
    printf("layout_host: batch layouts, lanes, views, decode tables, plan and many-inputs workspaces held at levels 1..9\n");
    return 0;
}
