// search_host.cpp -- the search without a device, built with g++ -fsanitize=address,undefined.
// (a) What one thread of search_tiles does, run thread by thread and tile by tile in the kernel's layout: the tile front that the
//     kernel itself compiles (banzai_amd/csrc/search_core.h: bzf_stage, bzf_match16, through BzfOne over the model LDS of scan_host.h), the
//     delimiter bits and the count of delimiters in front of a position, the counting pass, the scan of the tiles, the emitting
//     pass -- against a naive scan.  Every text is allocated as the kernel's contract states (16-byte aligned, up to the aligned
//     word that holds its last byte) and every other buffer has its exact size, so a read or a store outside is a sanitizer report.
// (b) The windows and the carry (banzai_amd/csrc/search_plan.h), with (a) as the device: blocks of seeded sizes expanded window by
//     window into a staging buffer that is allocated anew for every window, against brute force per output byte.
//
//   search_host <seed> <cases>     exit status 0: everything held
#define HOST_NAME "search_host"
#include "../../include/bzhip.h"
#include "scan_host.h"

static_assert(sizeof(bzh_hit) == sizeof(BzfHit) && sizeof(BzfHit) == 16, "a hit is two words");

struct Pattern {
    uint8_t pat[BZF_MAX_PATTERN];
    uint32_t plen, delim;
    bool records;
};

// search_window_run with the single pattern as the matcher: scan_host.h's model with BzfOne
static void window_run(const uint8_t *d, const BzfWindow &w, const Pattern &p, const BzfWalk &walk, std::vector<BzfHit> &out, uint64_t *hits, uint64_t *delims)
{
    search_run(d, w, BzfOne{{}, bzf_pattern(p.pat, p.plen, p.delim)}, p.records, walk, out, hits, delims);
}

// the truth: every start in [lo, hi - plen] of text[0, n), its record the delimiters in front of it
static std::vector<BzfHit> naive(const uint8_t *text, uint64_t n, const Pattern &p, uint64_t lo, uint64_t hi)
{
    std::vector<BzfHit> v;
    std::vector<uint64_t> cum(n + 1, 0);
    for (uint64_t i = 0; i < n; i++) cum[i + 1] = cum[i] + (text[i] == p.delim);
    hi = std::min(hi, n);
    for (uint64_t o = lo; o + p.plen <= hi; o++)
        if (memcmp(text + o, p.pat, p.plen) == 0) v.push_back(BzfHit{o, p.records ? cum[o] : 0});
    return v;
}

// ---- (a) raw bytes: one window, no staging --------------------------------------------------------------------------------
static uint64_t raw_case(const uint8_t *src, uint64_t n, const Pattern &p, uint64_t max)
{
    const Text text(src, n);
    const uint8_t *d = text.p;
    BzfWalk walk;
    walk.begin(p.plen, 0, max, 0, n, 0, 0);
    std::vector<BzfHit> out;
    uint64_t hits, delims;
    window_run(d, walk.window(n), p, walk, out, &hits, &delims);
    const std::vector<BzfHit> want = naive(d, n, p, 0, n);
    same_hits(out, want, hits, max, "raw", n);
    CHECK(!p.records || delims == (uint64_t)std::count(d, d + n, (uint8_t)p.delim), "raw (%llu): %llu delimiters", (unsigned long long)n,
          (unsigned long long)delims);
    return hits;
}

static void part_a()
{
    const uint64_t ns[] = {0, 1, 15, 16, 17, 4095, 4096, 4097, 8192, 12289};
    const uint32_t pls[] = {1, 2, 3, 4, 5, 16, 17, 255, 256};
    uint64_t found = 0, cases = 0;
    for (uint64_t n : ns)
        for (uint32_t plen : pls) {
            // seeded text over three letters and the delimiter, the pattern cut from it where it fits
            std::vector<uint8_t> text(n);
            for (auto &c : text) c = "ab\nc"[below(4)];
            Pattern p{{0}, plen, '\n', true};
            for (uint32_t j = 0; j < plen; j++) p.pat[j] = "ab\nc"[below(plen <= 5 ? 2 : 4)];
            if (n >= plen && below(4)) memcpy(p.pat, &text[below(n - plen + 1)], plen);
            found += raw_case(text.data(), n, p, ~0ull), cases++;
            // the fixed places: offset 0, ending at byte n - 1, across a thread edge, a wave edge, a tile edge
            const uint64_t edges[] = {0, n - plen, 16 - plen / 2, 1024 - plen / 2, 4096 - plen / 2, 4096 - 1, 8192 - plen + 1};
            if (n >= plen) {
                std::vector<uint8_t> t2(n, 'x');
                for (uint32_t j = 0; j < plen; j++) p.pat[j] = (uint8_t)('A' + j % 23);
                uint64_t planted = 0, last_end = 0;
                std::vector<uint64_t> es(edges, edges + 7);
                std::sort(es.begin(), es.end());
                for (uint64_t e : es)
                    if (e + plen <= n && e < n && (planted == 0 || e >= last_end)) memcpy(&t2[e], p.pat, plen), planted++, last_end = e + plen;
                const uint64_t h = raw_case(t2.data(), n, p, ~0ull);
                CHECK(h >= planted, "planted %llu, found %llu", (unsigned long long)planted, (unsigned long long)h);
                found += h, cases++;
                // one byte value everywhere: every start is a hit; and the delimiter equal to a pattern byte
                std::vector<uint8_t> t3(n, 'z');
                memset(p.pat, 'z', plen);
                p.delim = 'z';
                CHECK(raw_case(t3.data(), n, p, ~0ull) == n - plen + 1, "a buffer of one byte value");
                CHECK(raw_case(t3.data(), n, p, 3) == n - plen + 1, "a buffer of one byte value, three slots");
                p.records = false;
                raw_case(t3.data(), n, p, 0);
                cases += 3;
            } else {
                CHECK(raw_case(text.data(), n, p, ~0ull) == 0, "a pattern longer than the text has no hits");
            }
        }
    printf("raw: %llu cases held, %llu hits\n", (unsigned long long)cases, (unsigned long long)found);
}

// ---- (b) windows and the carry -----------------------------------------------------------------------------------------------
struct Ent {
    uint64_t out_len;
};

static void part_b(uint64_t cases)
{
    uint64_t windows = 0, carried = 0;
    for (uint64_t c = 0; c < cases; c++) {
        const size_t nb = 1 + below(7);
        std::vector<Ent> idx(nb);
        uint64_t total = 0;
        for (auto &e : idx) e.out_len = below(3) ? 1 + below(300) : 1 + below(9000), total += e.out_len;
        const uint32_t plen = below(3) ? 1 + (uint32_t)below(6) : 1 + (uint32_t)below(256);
        Pattern p{{0}, plen, '\n', below(4) != 0};
        for (uint32_t j = 0; j < plen; j++) p.pat[j] = "ab\n"[below(below(2) ? 3 : 1)];
        std::vector<uint8_t> truth(total);
        for (auto &ch : truth) ch = "ab\n"[below(3)];
        // a match and a delimiter on every block edge (every window edge is one)
        uint64_t edge = 0;
        for (size_t k = 0; k < nb; k++) {
            edge += idx[k].out_len;
            const uint64_t at = edge - std::min<uint64_t>(edge, below(plen + 1));
            if (at + plen <= total && below(4)) memcpy(&truth[at], p.pat, plen);
            if (edge < total && below(2)) truth[edge - below(2)] = '\n';
        }
        // a range of whole blocks' bytes from block `first` on, its ends anywhere: they cut matches at either end
        const size_t first = below(nb), last = first + 1 + below(nb - first);
        uint64_t start = 0, stop = 0;
        for (size_t k = 0; k < last; k++) (k < first ? start : stop) += idx[k].out_len;
        stop += start;
        const uint64_t lo = below(2) ? start : start + below(stop - start), hi = below(2) ? stop : lo + below(stop - lo + 1);
        const std::vector<BzfHit> want = naive(truth.data(), total, p, lo, hi);
        const uint64_t maxes[] = {~0ull, want.size(), want.size() ? want.size() - 1 : 0, 0, below(want.size() + 2)};
        const uint64_t max = maxes[below(5)];
        const uint64_t room = below(3) ? 1 + below(600) : 1 + below(20000);
        const size_t bmax = 1 + below(4);
        uint64_t rec_start = 0;
        for (uint64_t i = 0; i < start; i++) rec_start += truth[i] == '\n';
        BzfWalk walk;
        walk.begin(plen, BZF_FRONT, max, lo, hi, start, p.records ? rec_start : 0);
        std::vector<BzfHit> got((size_t)std::min<uint64_t>(max, want.size() + 8), BzfHit{~0ull, ~0ull});
        uint8_t carry[BZF_MAX_PATTERN];
        uint64_t at_out = start;
        for (size_t at = first; at < last;) {
            uint64_t bytes = 0;
            const size_t B = bzf_window_blocks(idx.data(), at, last, room, bmax, &bytes);
            CHECK(B >= 1 && B <= bmax && (B == 1 || bytes <= room), "a window of %zu blocks, %llu bytes", B, (unsigned long long)bytes);
            // SearchSink::room: a staging buffer of exactly these bytes, the carry in front of the window
            const Text staging(BZF_FRONT + bytes);
            uint8_t *stage = staging.p;
            memset(stage, poison_front, BZF_FRONT);
            if (walk.carry) memcpy(stage + BZF_FRONT - walk.carry, carry, (size_t)walk.carry);
            memcpy(stage + BZF_FRONT, &truth[at_out], (size_t)bytes);
            // SearchSink::window
            const BzfWindow w = walk.window(bytes);
            CHECK(w.n == BZF_FRONT + bytes && w.s_lo <= w.s_hi && w.s_lo >= BZF_FRONT - walk.carry && (w.s_hi == w.s_lo || w.s_hi + plen - 1 <= w.n),
                  "window");
            const uint64_t keep = walk.carry_after(bytes);
            CHECK(keep < plen && keep <= walk.carry + bytes, "carry");
            uint8_t next[BZF_MAX_PATTERN];
            memcpy(next, stage + w.n - keep, (size_t)keep);
            std::vector<BzfHit> out;
            uint64_t hits, delims;
            window_run(stage, w, p, walk, out, &hits, &delims);
            for (size_t i = 0; i < out.size(); i++) got.at((size_t)walk.rank + i) = out[i];
            walk.advance(bytes, hits, delims);
            memcpy(carry, next, (size_t)keep);
            CHECK(walk.carry == keep, "carry kept");
            at_out += bytes, at += B, windows++, carried += keep != 0;
        }
        same_hits(got, want, walk.rank, max, "windows", c);
    }
    printf("windows: %llu cases held, %llu windows, %llu carries\n", (unsigned long long)cases, (unsigned long long)windows,
           (unsigned long long)carried);
}

int main(int argc, char **argv)
{
    rng_state = argc > 1 ? strtoull(argv[1], nullptr, 10) * 0x9E3779B97F4A7C15ull + 1 : 1;
    const uint64_t cases = argc > 2 ? strtoull(argv[2], nullptr, 10) : 200;
    part_a();
    part_b(cases);
    return 0;
}
