// sync_host.cpp -- sync points on the one-lane CPU build of banzai_amd/csrc/decode_core.h, built by tests/test_sync_host.py with
// -fsanitize=address,undefined.  The GPU kernels (decode_block_sync_kernel, decode_header_kernel, decode_segment_kernel) compile
// the same header: the recorder's place in the symbol loop, the segment decode with its end check and the rule for ill-formed
// points are the very text that runs there.  For every block of every input stream this program
//   1. decodes serially with the recorder and prints the points;
//   2. decodes every segment on its own, from its point, into a heap buffer of exactly the bytes between its two points: the
//      joined segments must be the serial last column;
//   3. damages points (every single-bit flip of the 32 bytes in front of the MTF list of a few points, a sample of flips in the
//      MTF list, swapped and duplicated points): each must end in a status, or in bytes that differ from the serial column (so
//      that the block CRC catches it) -- and never in a sanitizer report.  This is where damage is thrown freely.
//
//   sync_host <cases> <interval> <report>   cases: [u32 n][n bytes]...
// report, one line each:
//   C <case> <blocks> <points>                                                 a case
//   E <bit_pos> <end_bit> <bytes of the last column> <stored crc> <stream> <level>   a block, in order
//   P <entry> <group> <bit_pos> <out_pos> <run> <run_weight> <512 hex digits>  a point, in order
//   D <point> <byte> <bit>     a single-bit flip that leaves the points well formed and is caught by a segment (BZH_E_DATA on the GPU)
//   S <damaged> <ill formed> <caught by a segment> <bytes differ>              the totals
// Exit status 0: all of it held; 3: an input did not decode; 4: joined segments differ; 5: a damaged point went unnoticed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/bzhip.h"
#include "../../banzai_amd/csrc/decode_core.h"

static_assert(sizeof(bzh_sync_point) == 288, "the sync point's layout");

struct HostRec {
    static constexpr bool ON = true;
    uint32_t interval;
    uint32_t entry;
    std::vector<bzh_sync_point> *out;
    void point(uint64_t pos, uint32_t gi, uint32_t nblock, uint32_t run, uint32_t run_weight, const uint8_t *mtf)
    {
        bzh_sync_point p;
        memset(&p, 0, sizeof p);
        p.bit_pos = pos;
        p.entry = entry;
        p.group = gi;
        p.out_pos = nblock;
        p.run = run;
        p.run_weight = run_weight;
        memcpy(p.mtf, mtf, 256);
        out->push_back(p);
    }
};

static BzdWork g_work, g_head;
static FILE *g_report;
static uint64_t g_damaged, g_ill, g_caught, g_differ;

static uint64_t peek48(const uint8_t *in, uint64_t n, uint64_t pos)
{
    BzdBits r;
    bzd_seek(r, in, n, pos);
    const uint64_t hi = bzd_get(r, 24);
    return hi << 24 | bzd_get(r, 24);
}

static BzdSyncState state_of(const bzh_sync_point &p)
{
    BzdSyncState s;
    s.bit_pos = p.bit_pos;
    s.group = p.group;
    s.out_pos = p.out_pos;
    s.run = p.run;
    s.run_weight = p.run_weight;
    s.mtf = p.mtf;
    return s;
}

// One block whose header g_head holds: segment j of its points pts[a .. b) runs from point a + j - 1 (j == 0: the header's state)
// to point a + j (j == b - a: the end of the block).
struct BlockCtx {
    const uint8_t *in;
    uint64_t n;
    BzdHdr h;
    uint32_t origptr;
    uint64_t first_bit;
    uint8_t mtf0[256];
    const uint8_t *L; // the serial last column
    uint32_t nblock;
};

// Decodes segment j into a heap buffer of exactly the bytes between its points.  0: it fits and its bytes are the serial column's;
// 1: a status (a kind or a miss); 2: no status, but bytes that differ from the serial column.
static int run_segment(const BlockCtx &b, const bzh_sync_point *pts, size_t a, size_t e, size_t j)
{
    BzdSyncState from, to;
    memset(&to, 0, sizeof to);
    if (j == 0) {
        from.bit_pos = b.first_bit;
        from.group = 0;
        from.out_pos = 0;
        from.run = 0;
        from.run_weight = 1;
        from.mtf = b.mtf0;
    } else {
        from = state_of(pts[a + j - 1]);
    }
    const bool has_to = a + j < e;
    if (has_to) to = state_of(pts[a + j]);
    // (the last segment's room is the block's size here: the buffer is exact in every segment)
    const uint32_t out_end = has_to ? to.out_pos : b.nblock;
    const size_t room = out_end >= from.out_pos ? (size_t)out_end - from.out_pos : 0;
    uint8_t *buf = (uint8_t *)malloc(room ? room : 1);
    BzdSegResult sr;
    bzd_decode_segment(g_head, g_head.sel, b.in, b.n, b.h.nin, b.h.nsel, b.origptr, from, has_to, to, b.nblock, buf, sr);
    int verdict = 0;
    if (sr.kind != BZD_OK || sr.miss != BZD_SEG_OK)
        verdict = 1;
    else if (from.out_pos + room > b.nblock || memcmp(buf, b.L + from.out_pos, room) != 0 || (!has_to && sr.nblock != b.nblock))
        verdict = 2;
    free(buf);
    return verdict;
}

// The points pts[a .. e) of one block, some of them damaged (orig: as recorded).  What the range decode would make of them.
enum Verdict { V_ILL, V_CAUGHT, V_DIFFER, V_UNNOTICED };
static Verdict judge(const BlockCtx &b, const std::vector<bzh_index_entry> &idx, const std::vector<bzh_sync_point> &pts,
                     const std::vector<bzh_sync_point> &orig, size_t a, size_t e)
{
    for (size_t i = a; i < e; i++)
        if (bzd_sync_point_check(idx.data(), idx.size(), pts.data(), i)) return V_ILL;
    bool differ = false;
    for (size_t j = 0; j <= e - a; j++) { // (a segment between two untouched points is step 2's: it fits)
        const bool from_same = j == 0 || memcmp(&pts[a + j - 1], &orig[a + j - 1], sizeof(bzh_sync_point)) == 0;
        const bool to_same = a + j >= e || memcmp(&pts[a + j], &orig[a + j], sizeof(bzh_sync_point)) == 0;
        if (from_same && to_same) continue;
        const int v = run_segment(b, pts.data(), a, e, j);
        if (v == 1) return V_CAUGHT;
        if (v == 2) differ = true;
    }
    return differ ? V_DIFFER : V_UNNOTICED;
}

static int damage_block(const BlockCtx &b, const std::vector<bzh_index_entry> &idx, std::vector<bzh_sync_point> &pts, size_t a, size_t e)
{
    if (a == e) return 0;
    const std::vector<bzh_sync_point> orig(pts);
    size_t picks[3] = {a, a + (e - a) / 2, e - 1};
    auto count = [&](Verdict v, const char *what, size_t i, uint32_t byte, uint32_t bit) {
        g_damaged++;
        if (v == V_ILL) g_ill++;
        if (v == V_CAUGHT) g_caught++;
        if (v == V_DIFFER) g_differ++;
        if (v == V_UNNOTICED) {
            fprintf(stderr, "sync_host: %s of point %zu (byte %u, bit %u) went unnoticed\n", what, i, byte, bit);
            return 5;
        }
        return 0;
    };
    for (int k = 0; k < 3; k++) {
        const size_t i = picks[k];
        if (k && i == picks[k - 1]) continue;
        uint8_t *raw = reinterpret_cast<uint8_t *>(&pts[i]);
        for (uint32_t byte = 0; byte < 32; byte++) // every bit in front of the MTF list
            for (uint32_t bit = 0; bit < 8; bit++) {
                raw[byte] ^= (uint8_t)(1u << bit);
                const Verdict v = judge(b, idx, pts, orig, a, e);
                raw[byte] ^= (uint8_t)(1u << bit);
                if (v == V_CAUGHT) fprintf(g_report, "D %zu %u %u\n", i, byte, bit);
                if (int rc = count(v, "a flip", i, byte, bit)) return rc;
            }
        for (uint32_t s = 0; s < 24; s++) { // a sample of the MTF list: its head, the bytes in use, the zeros behind them
            const uint32_t at = s < 8 ? s : (s < 16 ? (b.h.nin - 1 + 256 - (s - 8)) % 256 : (s * 53u) % 256), byte = 32 + at, bit = s % 8;
            raw[byte] ^= (uint8_t)(1u << bit);
            const Verdict v = judge(b, idx, pts, orig, a, e);
            raw[byte] ^= (uint8_t)(1u << bit);
            if (v == V_CAUGHT) fprintf(g_report, "D %zu %u %u\n", i, byte, bit);
            if (int rc = count(v, "an MTF flip", i, byte, bit)) return rc;
        }
        if (i + 1 < e) {
            std::swap(pts[i], pts[i + 1]);
            Verdict v = judge(b, idx, pts, orig, a, e);
            pts[i] = orig[i];
            pts[i + 1] = orig[i + 1];
            if (int rc = count(v, "a swap", i, 0, 0)) return rc;
            pts[i + 1] = pts[i];
            v = judge(b, idx, pts, orig, a, e);
            pts[i + 1] = orig[i + 1];
            if (int rc = count(v, "a duplicate", i, 0, 0)) return rc;
        }
    }
    return 0;
}

static int run_case(size_t ci, const uint8_t *in, uint64_t n, uint32_t interval)
{
    std::vector<bzh_index_entry> idx;
    std::vector<bzh_sync_point> pts;
    std::vector<uint8_t> L(900000);
    uint64_t at = 0;
    std::vector<size_t> first_point; // of every block
    std::vector<std::vector<uint8_t>> columns;
    uint32_t stream = 0;
    for (bool more = true; more;) {
        if (n - at < 4 || memcmp(in + at, "BZh", 3) != 0 || in[at + 3] < '1' || in[at + 3] > '9') return 3;
        const uint32_t level = (uint32_t)(in[at + 3] - '0'), block_max = 100000u * level;
        uint64_t pos = at * 8 + 32;
        for (;;) {
            if (pos + 48 > n * 8) return 3;
            const uint64_t magic = peek48(in, n, pos);
            BzdResult r;
            if (magic == BZD_FOOTER_MAGIC) {
                bzd_parse_footer(in, n, pos, r);
                if (r.kind) return 3;
                more = (r.follow & 0x100u) != 0;
                at = r.end_bit / 8;
                stream++;
                break;
            }
            if (magic != BZD_BLOCK_MAGIC) return 3;
            HostRec rec{interval, (uint32_t)idx.size(), &pts};
            first_point.push_back(pts.size());
            bzd_decode_block_rec(g_work, in, n, pos, block_max, L.data(), r, rec); // 1. serially, with the recorder
            if (r.kind) return 3;
            bzh_index_entry e;
            memset(&e, 0, sizeof e);
            e.bit_pos = pos;
            e.end_bit = r.end_bit;
            e.out_len = r.nblock; // (of the last column: the sizes behind the inverse RLE1 play no part here)
            e.crc = r.crc;
            e.stream = stream;
            e.level = level;
            idx.push_back(e);
            columns.emplace_back(L.begin(), L.begin() + r.nblock);
            pos = r.end_bit;
        }
    }
    first_point.push_back(pts.size());
    fprintf(g_report, "C %zu %zu %zu\n", ci, idx.size(), pts.size());
    for (const bzh_index_entry &e : idx)
        fprintf(g_report, "E %llu %llu %u %u %u %u\n", (unsigned long long)e.bit_pos, (unsigned long long)e.end_bit, e.out_len, e.crc, e.stream,
                e.level);
    for (const bzh_sync_point &p : pts) {
        fprintf(g_report, "P %u %u %llu %u %u %u ", p.entry, p.group, (unsigned long long)p.bit_pos, p.out_pos, p.run, p.run_weight);
        for (int k = 0; k < 256; k++) fprintf(g_report, "%02x", p.mtf[k]);
        fputc('\n', g_report);
    }
    for (size_t i = 0; i < pts.size(); i++)
        if (const char *what = bzd_sync_point_check(idx.data(), idx.size(), pts.data(), i)) {
            fprintf(stderr, "sync_host: recorded point %zu is ill formed: %s\n", i, what);
            return 4;
        }
    for (size_t k = 0; k < idx.size(); k++) {
        BlockCtx b;
        b.in = in;
        b.n = n;
        BzdBits r;
        bzd_seek(r, in, n, idx[k].bit_pos + 48);
        BzdResult hr;
        memset(&hr, 0, sizeof hr);
        if (!bzd_parse_header(g_head, r, hr, b.h)) return 3;
        b.origptr = hr.origptr;
        b.first_bit = r.pos;
        memcpy(b.mtf0, g_head.mtf, 256);
        b.L = columns[k].data();
        b.nblock = (uint32_t)columns[k].size();
        const size_t a = first_point[k], e = first_point[k + 1];
        for (size_t j = 0; j <= e - a; j++) // 2. every segment on its own
            if (run_segment(b, pts.data(), a, e, j) != 0) {
                fprintf(stderr, "sync_host: case %zu, block %zu: segment %zu does not fit or differs from the serial column\n", ci, k, j);
                return 4;
            }
        if (int rc = damage_block(b, idx, pts, a, e)) return rc; // 3.
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 4) {
        fprintf(stderr, "usage: sync_host <cases> <interval> <report>\n");
        return 2;
    }
    const uint32_t interval = (uint32_t)strtoul(argv[2], nullptr, 10);
    FILE *fi = fopen(argv[1], "rb");
    g_report = fopen(argv[3], "w");
    if (!fi || !g_report || interval < 1 || interval > 32767) return 2;
    for (size_t ci = 0;; ci++) {
        uint32_t n;
        if (fread(&n, 4, 1, fi) != 1) break;
        uint8_t *in = (uint8_t *)malloc(n ? n : 1); // an exact-size heap copy: a read past the case is a sanitizer report
        if (n && fread(in, 1, n, fi) != n) return 2;
        const int rc = run_case(ci, in, n, interval);
        free(in);
        if (rc) {
            fprintf(stderr, "sync_host: case %zu: exit status %d\n", ci, rc);
            return rc;
        }
    }
    fprintf(g_report, "S %llu %llu %llu %llu\n", (unsigned long long)g_damaged, (unsigned long long)g_ill, (unsigned long long)g_caught,
            (unsigned long long)g_differ);
    fclose(fi);
    return fclose(g_report) ? 2 : 0;
}
