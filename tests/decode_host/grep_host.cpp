// grep_host.cpp -- the grep without a device, built with g++ -fsanitize=address,undefined.
// (a) What one thread, one tile and the scan of grep_tiles / grep_scan do, run thread by thread and tile by tile in the kernel's
//     layout: the tile front that the kernel itself compiles (banzai_amd/csrc/search_core.h: bzf_stage, bzf_match16, through BzfOne over the model
//     LDS of scan_host.h), then banzai_amd/csrc/grep_core.h -- every phase for thread 0 .. 255 where the kernel has a barrier, the
//     counting pass, the scan, the gather -- against a naive split-and-find.  Every text is allocated as the kernel's contract
//     states (16-byte aligned, up to the aligned word that holds its last byte) and every other buffer has its exact size, so a
//     read or a store outside is a sanitizer report.
// (b) The windows and the carry (banzai_amd/csrc/grep_plan.h), with (a) as the device: blocks of seeded sizes expanded window by
//     window into a staging buffer that is allocated anew for every window, against the same naive split-and-find.
//
//   grep_host <seed> <cases>     exit status 0: everything held
#define HOST_NAME "grep_host"
#include "../../include/bzhip.h"
#include "scan_host.h"

struct Pattern {
    uint8_t pat[BZF_MAX_PATTERN];
    uint32_t plen, delim, invert;
};
static uint8_t slack_of(const Pattern &p) { return p.delim == 0xEE ? 0xED : 0xEE; } // (the letters are 'a' .. 'd')

// ---- the truth: split at the delimiter, find in every record ("a match belongs to the record of its first byte") ---------------
static GrepTruth naive(const Bytes &text, const Pattern &p)
{
    GrepTruth tr;
    const uint64_t n = text.size();
    uint64_t start = 0, rec = 0;
    auto close = [&](uint64_t end) { // the record [start, end)
        bool hit = false;
        for (uint64_t s = start; s < end && !hit; s++) hit = s + p.plen <= n && memcmp(&text[s], p.pat, p.plen) == 0;
        if (hit != (p.invert != 0)) {
            tr.ent.push_back(BzgEntry{rec, start, end - start, tr.out.size()});
            tr.out.insert(tr.out.end(), text.begin() + start, text.begin() + end);
        }
        rec++;
        start = end;
    };
    for (uint64_t i = 0; i < n; i++)
        if (text[i] == p.delim) close(i + 1);
    if (start < n) close(n);
    tr.nrecords = rec;
    return tr;
}

// ---- (a) the device: scan_host.h's model with BzfOne, the single pattern ----------------------------------------------------------
// one call: `blocks` lists the sizes of the windows' new bytes (empty: the raw call, one window over the text itself)
static void run_call(const Bytes &text, const Pattern &p, const std::vector<uint64_t> &blocks, int out_kind, int ent_kind, const GrepTruth &tr, uint64_t *carry_peak,
                     uint64_t *windows)
{
    const BzfOne m{{}, bzf_pattern(p.pat, p.plen, p.delim)};
    grep_call(text, tr, [&](const BzgWindow &) { return m; }, p.plen, p.invert, slack_of(p), blocks, out_kind, ent_kind, carry_peak, windows);
}

// ---- texts -------------------------------------------------------------------------------------------------------------------------
static void plant(Bytes &text, uint64_t at, const Pattern &p)
{
    if (at + p.plen <= text.size()) memcpy(&text[at], p.pat, p.plen);
}
static Pattern pattern(uint32_t plen, uint32_t delim, uint32_t invert, int kind) // kind 0: letters; 1: begins with the delimiter; 2: ends with it; 3: both
{
    Pattern p{};
    p.plen = plen, p.delim = delim, p.invert = invert;
    for (uint32_t j = 0; j < plen; j++) p.pat[j] = (uint8_t)('a' + below(2));
    if (kind & 1) p.pat[0] = (uint8_t)delim;
    if (kind & 2) p.pat[plen - 1] = (uint8_t)delim;
    return p;
}
// density: one delimiter in `density` bytes (0: none)
static Bytes letters(uint64_t n, uint32_t delim, uint64_t density)
{
    Bytes t(n);
    for (auto &b : t) b = density && below(density) == 0 ? (uint8_t)delim : (uint8_t)('a' + below(2));
    return t;
}

static uint64_t seen_selected, seen_left; // records the truth selects and leaves out
static void raw_case(const Bytes &text, const Pattern &p, uint64_t *runs)
{
    const GrepTruth tr = naive(text, p);
    seen_selected += tr.ent.size(), seen_left += tr.nrecords - tr.ent.size();
    run_call(text, p, {}, 2, 2, tr, nullptr, nullptr);
    (*runs)++;
}

static void raw_cases()
{
    static const uint64_t ns[] = {0, 1, 15, 16, 17, 4095, 4096, 4097, 8192, 12289};
    static const uint32_t plens[] = {1, 2, 3, 4, 5, 16, 17, 255, 256};
    uint64_t runs = 0;
    for (uint64_t n : ns)
        for (uint32_t plen : plens)
            for (uint32_t invert = 0; invert < 2; invert++) {
                const uint32_t delim = '\n';
                for (int kind = 0; kind < 4; kind++) { // seeded text of every delimiter density, the pattern planted at the edges
                    const Pattern p = pattern(plen, delim, invert, kind);
                    static const uint64_t dens[] = {0, 3, 40, 3000};
                    Bytes text = letters(n, delim, dens[below(4)]);
                    for (uint64_t edge : {(uint64_t)0, (uint64_t)16, (uint64_t)1024, (uint64_t)4096, (uint64_t)8192, n})
                        if (below(2)) plant(text, edge >= plen / 2 ? edge - plen / 2 : 0, p);
                    if (n >= plen && below(2)) plant(text, n - plen, p);
                    raw_case(text, p, &runs);
                }
                const Pattern p = pattern(plen, delim, invert, 0);
                // a delimiter as the last byte of a thread, of a wave and of a tile, and as the first byte of the next; a tail that is
                // empty and one that is not
                for (uint64_t edge : {(uint64_t)16, (uint64_t)1024, (uint64_t)4096})
                    for (uint64_t at : {edge - 1, edge}) {
                        Bytes text = letters(n, delim, 0);
                        if (at < n) text[at] = (uint8_t)delim;
                        if (below(2) && n) text[n - 1] = (uint8_t)delim;
                        plant(text, below(n + 1), p);
                        raw_case(text, p, &runs);
                    }
                // a record over three tiles with its only hit in the first, the middle and the last tile
                if (n == 12289)
                    for (uint64_t at : {(uint64_t)300, (uint64_t)5000, (uint64_t)9000}) {
                        Bytes text(n, 'c');
                        text[100] = text[101] = (uint8_t)delim, text[12000] = (uint8_t)delim;
                        plant(text, at, p);
                        raw_case(text, p, &runs);
                    }
                // delimiters only (empty records); the pattern is the delimiter; no delimiter at all
                {
                    Bytes text(n, (uint8_t)delim);
                    raw_case(text, p, &runs);
                    Pattern q = p;
                    memset(q.pat, (int)delim, q.plen);
                    raw_case(text, q, &runs);
                    raw_case(letters(n, delim, 3), q, &runs);
                    raw_case(letters(n, delim, 0), p, &runs);
                }
                // selected output that starts at every residue modulo 16: a first record of 1 .. 16 bytes, then the rest
                for (uint64_t first = 1; first <= 16 && first < n; first++) {
                    Bytes text = letters(n, delim, 30);
                    for (uint64_t j = 0; j < first; j++) text[j] = 'c';
                    text[first - 1] = (uint8_t)delim;
                    Pattern q = pattern(1, delim, invert, 0);
                    q.pat[0] = invert ? 'z' : 'c'; // (the first record is selected either way)
                    if (first == 1) q.pat[0] = invert ? 'z' : (uint8_t)delim;
                    raw_case(text, q, &runs);
                }
            }
    // more tiles than the scan has threads: every thread of grep_scan walks a run of tiles, in batches and a rest
    for (uint64_t tiles : {(uint64_t)700, (uint64_t)2400})
        for (uint32_t invert = 0; invert < 2; invert++) {
            const uint64_t n = tiles * BZF_TILE + 77;
            const Pattern p = pattern(3, '\n', invert, invert ? 2 : 0);
            Bytes text = letters(n, '\n', invert ? 30000 : 900);
            for (uint64_t at = 5000; at + 3 < n; at += 70001) plant(text, at, p);
            raw_case(text, p, &runs);
        }
    CHECK(seen_selected > runs && seen_left > runs, "the cases select and leave out: %llu, %llu", (unsigned long long)seen_selected,
          (unsigned long long)seen_left);
    printf("raw: %llu calls held (%llu records selected, %llu left out)\n", (unsigned long long)runs, (unsigned long long)seen_selected,
           (unsigned long long)seen_left);
}

static void window_cases(uint64_t cases)
{
    uint64_t carry_peak = 0, most_windows = 0, over = 0;
    for (uint64_t c = 0; c < cases; c++) {
        // the blocks, and the windows of 1 to 4 of them
        const uint32_t nb = 1 + (uint32_t)below(7);
        std::vector<uint64_t> blocks, wins;
        uint64_t n = 0;
        for (uint32_t k = 0; k < nb; k++) blocks.push_back(1 + below(below(4) ? 600 : 9000)), n += blocks.back();
        for (uint32_t k = 0; k < nb;) {
            uint64_t sum = 0;
            const uint32_t take = 1 + (uint32_t)below(4);
            for (uint32_t j = 0; j < take && k < nb; j++, k++) sum += blocks[k];
            wins.push_back(sum);
        }
        static const uint32_t plens[] = {1, 2, 3, 4, 5, 16, 17, 255, 256};
        const uint32_t delim = below(4) ? '\n' : (uint32_t)below(256);
        Pattern p = pattern(plens[below(9)], delim, (uint32_t)below(2), (int)below(4));
        static const uint64_t dens[] = {0, 3, 40, 700, 20000};
        Bytes text = letters(n, delim, dens[below(5)]);
        if (delim == 'a' || delim == 'b')
            for (auto &b : text) b = b == delim ? b : (uint8_t)('c' + (b & 1)); // (letters that are not the delimiter)
        // a window edge with a carry of 1, 511, 512, 513 or 5,000 bytes behind its last delimiter; the only hit in that carry, or
        // across the edge
        uint64_t edge = 0;
        for (size_t k = 0; k + 1 < wins.size(); k++) {
            edge += wins[k];
            static const uint64_t carries[] = {1, 511, 512, 513, 5000};
            const uint64_t cy = carries[below(5)];
            if (below(2) || edge < cy + 1) continue;
            for (uint64_t j = edge - cy; j < edge; j++)
                if (text[j] == delim) text[j] = 'c';
            text[edge - cy - 1] = (uint8_t)delim;
            const int how = (int)below(3);
            if (how == 0 && cy >= p.plen) plant(text, edge - cy + below(cy - p.plen + 1), p);
            if (how == 1) plant(text, edge >= 1 + below(p.plen) ? edge - 1 - below(p.plen) : 0, p);
        }
        edge = 0;
        for (size_t k = 0; k + 1 < wins.size(); k++) { // a match across the window edge
            edge += wins[k];
            if (below(3) == 0) plant(text, edge >= p.plen / 2 ? edge - p.plen / 2 : 0, p);
        }
        if (below(4) == 0) { // a text without the pattern's letters but for one planted hit
            for (auto &b : text) b = b == delim ? b : 'c';
            plant(text, below(n), p);
        }
        const GrepTruth tr = naive(text, p);
        const int out_kind = (int)below(5), ent_kind = (int)below(5);
        uint64_t windows = 0;
        run_call(text, p, wins, out_kind, ent_kind, tr, &carry_peak, &windows);
        run_call(text, p, wins, 2, 2, tr, nullptr, nullptr); // (and with the exact rooms)
        most_windows = std::max(most_windows, windows);
        over += (out_kind >= 3 && !tr.out.empty()) || (ent_kind >= 3 && !tr.ent.empty());
    }
    CHECK(carry_peak >= 5000 && most_windows >= 4 && over > cases / 20, "the cases reach the edges: carry %llu, windows %llu, too small %llu",
          (unsigned long long)carry_peak, (unsigned long long)most_windows, (unsigned long long)over);
    printf("windows: %llu cases held (longest carry %llu, most windows %llu, %llu with too little room)\n", (unsigned long long)cases,
           (unsigned long long)carry_peak, (unsigned long long)most_windows, (unsigned long long)over);
}

int main(int argc, char **argv)
{
    rng_state = (argc > 1 ? strtoull(argv[1], nullptr, 10) : 1) * 0x9E3779B97F4A7C15ull + 1;
    const uint64_t cases = argc > 2 ? strtoull(argv[2], nullptr, 10) : 200;
    static_assert(sizeof(bzh_grep_entry) == sizeof(BzgEntry) && sizeof(BzgEntry) == 32, "an entry is four words");
    raw_cases();
    window_cases(cases);
    return 0;
}
