// stream_index_host.cpp -- the host side of an index written while its stream is (banzai_amd/csrc/stream_index.h), built with
// g++ -fsanitize=address,undefined:
//   * bzs_base / bzs_rebase / bzs_take against a restatement.  A stream is laid out once in absolute coordinates: that is what
//     bzh_encode_index would return.  It is then cut into passes as bzh_stream_feed cuts it -- a pass packs from the bit
//     phase = (stream bits so far) % 32 of a buffer of its own and numbers its blocks and bytes from 0; some passes find no
//     final block --, each pass's arrays are rebased and appended, and takes with random room move them out.  What was taken
//     must be the absolute arrays, byte for byte.  Streams start at bit positions up to 2^40 and every phase 0..31 occurs.
//   * bzs_blob_write / bzs_blob_read on random indexes (exact-size heap buffers, so a read past a blob is a sanitizer report):
//     the round trip, BZH_E_CAP with both counts, every truncation, every header bit and a sample of body bits flipped, and
//     random bytes behind either magic.
//
//   stream_index_host <seed> <cases>     exit status 0: everything held
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/bzhip.h"
#include "../../banzai_amd/csrc/stream_index.h"

static uint64_t rng_state;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}
static uint64_t below(uint64_t n) { return n ? rnd() % n : 0; }

#define CHECK(cond, ...)                                        \
    do {                                                        \
        if (!(cond)) {                                          \
            fprintf(stderr, "stream_index_host: %s: ", #cond);  \
            fprintf(stderr, __VA_ARGS__);                       \
            fprintf(stderr, "\n");                              \
            exit(1);                                            \
        }                                                       \
    } while (0)

static bzh_sync_point make_point(uint64_t bit, uint32_t entry, uint32_t group)
{
    bzh_sync_point p;
    memset(&p, 0, sizeof p);
    p.bit_pos = bit;
    p.entry = entry;
    p.group = group;
    p.out_pos = (uint32_t)below(900000);
    p.run = (uint32_t)below(4);
    p.run_weight = 1u << below(3);
    for (int k = 0; k < 256; k++) p.mtf[k] = (uint8_t)rnd();
    return p;
}

static uint32_t phases_seen = 0;

// ---- rebase --------------------------------------------------------------------------------------------------------------
static void rebase_case()
{
    // the stream in absolute coordinates; entry numbers and out_off start at arbitrary values, as in the middle of a long stream
    const uint64_t bits0 = below(4) == 0 ? 32 : (below(2) ? ((uint64_t)1 << 32) + below((uint64_t)1 << 40) : 32 + below(100000));
    const uint64_t out0 = below(3) == 0 ? 0 : below((uint64_t)1 << 45);
    const uint32_t ent0 = below(3) == 0 ? 0 : (uint32_t)below(1u << 20);
    const uint32_t npass = 1 + (uint32_t)below(9);
    std::vector<bzh_index_entry> abs_e;
    std::vector<bzh_sync_point> abs_p;
    std::vector<bzh_index_entry> got_e, pend_e;
    std::vector<bzh_sync_point> got_p, pend_p;
    uint64_t bits = bits0, consumed = out0, blocks = ent0;
    for (uint32_t ps = 0; ps < npass; ps++) {
        const uint32_t phase = (uint32_t)(bits & 31u);
        phases_seen |= 1u << phase;
        const uint64_t word0 = bits / 32 * 32; // the stream bit that is bit 0 of the pass's buffer
        const uint32_t nb = below(4) == 0 ? 0 : 1 + (uint32_t)below(5); // (a pass with no final block adds nothing)
        std::vector<bzh_index_entry> pe;
        std::vector<bzh_sync_point> pp;
        uint64_t cur = bits, off = consumed;
        for (uint32_t b = 0; b < nb; b++) {
            const uint64_t len = 174 + below(below(6) == 0 ? 7000000 : 3000);
            const uint32_t raw = 1 + (uint32_t)below(900000);
            bzh_index_entry a{cur, cur + len, off, raw, (uint32_t)rnd(), 0, 1 + (uint32_t)below(9)};
            abs_e.push_back(a);
            bzh_index_entry l = a; // what the pass's own EncIndex holds
            l.bit_pos = cur - word0;
            l.end_bit = cur + len - word0;
            l.out_off = off - consumed;
            pe.push_back(l);
            CHECK(b > 0 || l.bit_pos == phase, "a pass packs from its phase");
            const uint32_t np = (uint32_t)below(4);
            for (uint32_t q = 0; q < np; q++) {
                const uint64_t at = cur + 1 + (len - 2) * (q + 1) / (np + 1);
                bzh_sync_point ap = make_point(at, (uint32_t)(blocks + b), (q + 1) * 7);
                abs_p.push_back(ap);
                bzh_sync_point lp = ap;
                lp.bit_pos = at - word0;
                lp.entry = b;
                pp.push_back(lp);
            }
            cur += len;
            off += raw;
        }
        // the collect step of bzh_stream_feed
        if (!pe.empty()) {
            const size_t e0 = pend_e.size(), p0 = pend_p.size();
            pend_e.insert(pend_e.end(), pe.begin(), pe.end());
            pend_p.insert(pend_p.end(), pp.begin(), pp.end());
            bzs_rebase(bzs_base(bits, consumed, blocks), pend_e.data() + e0, pe.size(), pend_p.data() + p0, pp.size());
        }
        bits = cur;
        consumed = off;
        blocks += nb;
        // a take: with room enough, or one short in either array
        if (below(3) != 0 || ps + 1 == npass) {
            const size_t ne = pend_e.size(), np = pend_p.size();
            size_t c = 99, n = 99;
            if (below(2) && (ne || np)) {
                const bool short_e = ne && (np == 0 || below(2));
                std::vector<bzh_index_entry> be(short_e ? ne - 1 : ne);
                std::vector<bzh_sync_point> bp(short_e ? np : np - 1);
                CHECK(!bzs_take(pend_e, pend_p, be.data(), be.size(), &c, bp.data(), bp.size(), &n), "a short take must fail");
                CHECK(c == ne && n == np && pend_e.size() == ne && pend_p.size() == np, "a short take sets the counts and removes nothing");
            }
            std::vector<bzh_index_entry> be(ne);
            std::vector<bzh_sync_point> bp(np);
            CHECK(bzs_take(pend_e, pend_p, be.data(), ne, &c, bp.data(), np, &n), "a take with room");
            CHECK(c == ne && n == np && pend_e.empty() && pend_p.empty(), "a take moves everything out");
            got_e.insert(got_e.end(), be.begin(), be.end());
            got_p.insert(got_p.end(), bp.begin(), bp.end());
        }
    }
    CHECK(got_e.size() == abs_e.size() && got_p.size() == abs_p.size(), "%zu / %zu entries, %zu / %zu points", got_e.size(), abs_e.size(),
          got_p.size(), abs_p.size());
    CHECK(abs_e.empty() || memcmp(got_e.data(), abs_e.data(), abs_e.size() * sizeof(bzh_index_entry)) == 0, "entries differ");
    CHECK(abs_p.empty() || memcmp(got_p.data(), abs_p.data(), abs_p.size() * sizeof(bzh_sync_point)) == 0, "points differ");
}

// ---- blobs ---------------------------------------------------------------------------------------------------------------
// An independent CRC-32: bit by bit.
static uint32_t crc_slow(const uint8_t *p, size_t n)
{
    uint32_t c = 0xFFFFFFFFu;
    for (size_t k = 0; k < n; k++) {
        c ^= p[k];
        for (int b = 0; b < 8; b++) c = (c & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
    }
    return ~c;
}

struct Read {
    int st;
    std::vector<bzh_index_entry> e;
    std::vector<bzh_sync_point> p;
    size_t count, npts;
    uint32_t interval;
    uint64_t consumed;
};
// the blob in a heap buffer of exactly its size; arrays of exactly the room given
static Read read_blob(const std::vector<uint8_t> &blob, size_t max, size_t max_pts)
{
    uint8_t *b = (uint8_t *)malloc(blob.size() ? blob.size() : 1);
    if (!blob.empty()) memcpy(b, blob.data(), blob.size());
    Read r;
    r.e.resize(max);
    r.p.resize(max_pts);
    r.st = bzs_blob_read(b, blob.size(), max ? r.e.data() : nullptr, max, &r.count, max_pts ? r.p.data() : nullptr, max_pts, &r.npts,
                         &r.interval, &r.consumed);
    free(b);
    return r;
}

static void blob_case(bool big)
{
    const size_t count = big ? 300 : below(4), npts = below(3) == 0 ? 0 : (big ? 2000 + below(2000) : below(5));
    const uint32_t interval = below(3) == 0 ? 0 : (below(2) ? 1 : (below(2) ? 256 : 1 + (uint32_t)below(32767)));
    const uint64_t consumed = rnd() >> below(40);
    std::vector<bzh_index_entry> e(count);
    std::vector<bzh_sync_point> p(interval ? npts : 0);
    for (auto &x : e) x = bzh_index_entry{rnd(), rnd(), rnd(), (uint32_t)rnd(), (uint32_t)rnd(), (uint32_t)rnd(), (uint32_t)rnd()};
    for (auto &x : p) x = make_point(rnd(), (uint32_t)rnd(), (uint32_t)rnd());
    const size_t need = bzs_blob_size(e.size(), p.size(), interval);
    CHECK(need == (interval ? 40 + 32 + 40 * e.size() + 288 * p.size() : 32 + 40 * e.size()), "size %zu", need);
    std::vector<uint8_t> blob(need);
    size_t got = 0;
    if (need > 0) {
        std::vector<uint8_t> small(need - 1);
        CHECK(bzs_blob_write(e.data(), e.size(), p.data(), p.size(), interval, consumed, small.data(), small.size(), &got) == BZH_E_CAP && got == need,
              "a buffer one byte short");
    }
    CHECK(bzs_blob_write(e.data(), e.size(), p.data(), p.size(), interval, consumed, blob.data(), blob.size(), &got) == BZH_OK && got == need, "write");
    if (interval) {
        uint8_t head[40];
        memcpy(head, blob.data(), 40);
        memset(head + 32, 0, 4);
        std::vector<uint8_t> all(head, head + 40);
        all.insert(all.end(), blob.begin() + 40, blob.end());
        CHECK(bzs_get32(blob.data() + 32) == crc_slow(all.data(), all.size()), "the CRC field against a bitwise CRC-32");
    }
    Read r = read_blob(blob, e.size(), p.size());
    CHECK(r.st == BZH_OK && r.count == e.size() && r.npts == p.size() && r.interval == interval && r.consumed == consumed, "read: status %d", r.st);
    CHECK(e.empty() || memcmp(r.e.data(), e.data(), e.size() * 40) == 0, "entries come back");
    CHECK(p.empty() || memcmp(r.p.data(), p.data(), p.size() * 288) == 0, "points come back");
    if (!e.empty()) {
        r = read_blob(blob, e.size() - 1, p.size());
        CHECK(r.st == BZH_E_CAP && r.count == e.size() && r.npts == p.size(), "entries one short: both counts");
    }
    if (!p.empty()) {
        r = read_blob(blob, e.size(), p.size() - 1);
        CHECK(r.st == BZH_E_CAP && r.count == e.size() && r.npts == p.size(), "points one short: both counts");
    }
    // damage: every truncation of a small blob (a sample of a big one), bits flipped
    for (size_t cut = 0; cut < need; cut += big ? 1 + below(40000) : 1) {
        std::vector<uint8_t> t(blob.begin(), blob.begin() + cut);
        CHECK(read_blob(t, e.size(), p.size()).st == BZH_E_DATA, "a blob cut to %zu of %zu bytes", cut, need);
    }
    {
        std::vector<uint8_t> t = blob;
        t.push_back(0);
        CHECK(read_blob(t, e.size(), p.size()).st == BZH_E_DATA, "a byte too many");
    }
    const size_t head = interval ? 40 : 24; // (a block index: `consumed`, bytes 24..31, is data like the entries -- no CRC guards it)
    for (size_t bit = 0; bit < head * 8; bit += big ? 1 + below(16) : 1) { // (every bit of a small blob's header)
        std::vector<uint8_t> t = blob;
        t[bit / 8] ^= (uint8_t)(1u << (bit % 8));
        CHECK(read_blob(t, e.size(), p.size()).st == BZH_E_DATA, "header bit %zu flipped", bit);
    }
    if (interval)
        for (int k = 0; k < (big ? 8 : 64) && need > 40; k++) {
            std::vector<uint8_t> t = blob;
            const size_t bit = 40 * 8 + below((need - 40) * 8);
            t[bit / 8] ^= (uint8_t)(1u << (bit % 8));
            CHECK(read_blob(t, e.size(), p.size()).st == BZH_E_DATA, "body bit %zu flipped", bit);
        }
    // random bytes behind a magic: any status, no access outside the blob
    for (int k = 0; k < 8; k++) {
        std::vector<uint8_t> t(below(200));
        for (auto &x : t) x = (uint8_t)rnd();
        if (t.size() >= 8) memcpy(t.data(), below(2) ? BZS_IDX_MAGIC : BZS_SYN_MAGIC, 8);
        if (t.size() >= 12 && below(2)) bzs_put32(t.data() + 8, 1);
        const int st = read_blob(t, 8, 8).st;
        CHECK(st == BZH_E_DATA || st == BZH_E_CAP || st == BZH_OK, "status %d", st);
    }
}

static void blob_fixed()
{
    size_t got = 0, c = 0, n = 0;
    uint32_t iv = 0;
    uint64_t cons = 0;
    uint8_t buf[128];
    bzh_sync_point pt = make_point(1, 0, 1);
    CHECK(bzs_blob_size(0, 1, 0) == 0 && bzs_blob_size(0, 0, 32768) == 0 && bzs_blob_size(SIZE_MAX / 8, 0, 0) == 0 &&
              bzs_blob_size(1, SIZE_MAX / 100, 5) == 0, "sizes that are refused");
    CHECK(bzs_blob_write(nullptr, 0, &pt, 1, 0, 0, buf, sizeof buf, &got) == BZH_E_ARG, "points without an interval");
    CHECK(bzs_blob_write(nullptr, 0, nullptr, 0, 40000, 0, buf, sizeof buf, &got) == BZH_E_ARG, "an interval above 32767");
    CHECK(bzs_blob_write(nullptr, 1, nullptr, 0, 0, 0, buf, sizeof buf, &got) == BZH_E_ARG, "a null array with a count");
    CHECK(bzs_blob_write(nullptr, 0, nullptr, 0, 0, 7, buf, sizeof buf, &got) == BZH_OK && got == 32, "the empty block index");
    CHECK(bzs_blob_read(buf, 32, nullptr, 0, &c, nullptr, 0, &n, &iv, &cons) == BZH_OK && c == 0 && n == 0 && iv == 0 && cons == 7, "and back");
    CHECK(bzs_blob_read(buf, 32, nullptr, 0, nullptr, nullptr, 0, &n, &iv, &cons) == BZH_E_ARG, "a null count");
    CHECK(bzs_blob_write(nullptr, 0, nullptr, 0, 16, 9, buf, sizeof buf, &got) == BZH_OK && got == 72, "the empty sync index");
    CHECK(bzs_blob_read(buf, 72, nullptr, 0, &c, nullptr, 0, &n, &iv, &cons) == BZH_OK && c == 0 && n == 0 && iv == 16 && cons == 9, "and back");
    // counts that would overflow the size arithmetic, under a valid CRC
    bzs_put64(buf + 24, UINT64_MAX / 288 + 1);
    bzs_put32(buf + 32, 0);
    bzs_put32(buf + 32, bzs_crc32(0, buf, 72));
    CHECK(bzs_blob_read(buf, 72, nullptr, 0, &c, nullptr, 0, &n, &iv, &cons) == BZH_E_DATA, "2^64 / 288 points");
    CHECK(bzs_crc32(0, (const uint8_t *)"123456789", 9) == 0xCBF43926u, "the CRC-32 check value");
    CHECK(bzs_crc32(bzs_crc32(0, (const uint8_t *)"1234", 4), (const uint8_t *)"56789", 5) == 0xCBF43926u, "continued");
}

int main(int argc, char **argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: stream_index_host <seed> <cases>\n");
        return 2;
    }
    rng_state = strtoull(argv[1], nullptr, 10) * 0x9E3779B97F4A7C15ull + 1;
    const long cases = atol(argv[2]);
    blob_fixed();
    for (long k = 0; k < cases; k++) rebase_case();
    CHECK(cases < 200 || phases_seen == 0xFFFFFFFFu, "phases seen: %08x", phases_seen);
    for (long k = 0; k < cases / 10 + 1; k++) blob_case(k % 64 == 63);
    printf("stream_index_host: %ld rebase cases and %ld blob cases held\n", cases, cases / 10 + 1);
    return 0;
}
