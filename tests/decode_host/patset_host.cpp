// patset_host.cpp -- search and grep for a set of patterns without a device, built with g++ -fsanitize=address,undefined.
// (a) The compile of banzai_amd/csrc/patset_plan.h against a naive matcher: equal patterns, prefixes, suffixes, every byte value,
//     the state bound, what folds and what does not.
// (b) The matcher of banzai_amd/csrc/patset_core.h -- BzmMatcher, the kernels' own text -- thread by thread and tile by tile in
//     the kernels' layout over a model of the LDS: both passes of search_tiles and the scan between them, both passes of
//     grep_tiles with grep_core.h's phases and scan.  The table has its exact size, every text is allocated as the kernels'
//     contract states (tile_host.h: Text), every other buffer has its exact size: a read or a store outside is a sanitizer report.
// (c) The windows: BzmSetWalk (search_plan.h) and BzgWalk (grep_plan.h) with (b) as the device, against brute force per byte.
//
//   patset_host <seed> <cases>     exit status 0: everything held
#define HOST_NAME "patset_host"
#include <string>

#include "../../include/bzhip.h"
#include "../../banzai_amd/csrc/patset_plan.h"
#include "scan_host.h"

typedef std::vector<Bytes> Pats;

static_assert(sizeof(bzh_set_hit) == sizeof(BzmHit) && sizeof(BzmHit) == 24, "a set's hit is three words");
static_assert(sizeof(bzh_grep_entry) == sizeof(BzgEntry), "an entry is four words");

// ---- a compiled set as the device holds it, and the naive matcher ----------------------------------------------------------------
struct Set {
    BzmPlan plan;
    uint8_t *cls = nullptr;
    uint16_t *first = nullptr, *table = nullptr;
    uint32_t *pat_no = nullptr;
    bool fold = false;
    std::vector<std::pair<Bytes, uint32_t>> distinct; // the folded patterns, each with its number, by length
    bool ok = false;
    std::string why;
    Set(const Pats &pats, unsigned flags)
    {
        std::vector<const uint8_t *> ptr;
        std::vector<size_t> len;
        for (const Bytes &p : pats) ptr.push_back(p.data()), len.push_back(p.size());
        char err[200] = "";
        ok = bzm_compile(ptr.data(), len.data(), pats.size(), flags, plan, err, sizeof err);
        why = err;
        if (!ok) return;
        fold = (flags & BZM_FOLD_ASCII) != 0;
        cls = exact(plan.cls, 256), first = exact(plan.first, 256);
        table = exact(plan.table.data(), plan.table.size()), pat_no = exact(plan.pat_no.data(), plan.pat_no.size());
        for (uint32_t i = 0; i < pats.size(); i++) {
            Bytes f = pats[i];
            for (auto &b : f) b = bzm_fold(b, fold);
            bool seen = false;
            for (auto &d : distinct) seen |= d.first == f;
            if (!seen) distinct.push_back({f, i});
        }
        std::stable_sort(distinct.begin(), distinct.end(), [](const auto &a, const auto &b) { return a.first.size() < b.first.size(); });
    }
    ~Set() { free(cls), free(first), free(table), free(pat_no); }
    Set(const Set &) = delete;
    BzmMatcher matcher(uint32_t delim, uint64_t lim) const
    {
        return BzmMatcher{BzmSet{cls, first, table, pat_no, plan.classes, (uint32_t)plan.distinct, plan.max_len, delim, lim}};
    }
    bool at(const uint8_t *text, uint64_t o, uint64_t lim, const Bytes &p) const // the rule
    {
        if (o + p.size() > lim) return false;
        for (size_t j = 0; j < p.size(); j++)
            if (bzm_fold(text[o + j], fold) != p[j]) return false;
        return true;
    }
    bool any_at(const uint8_t *text, uint64_t o, uint64_t lim) const
    {
        for (auto &d : distinct)
            if (at(text, o, lim, d.first)) return true;
        return false;
    }
    // every pair with lo <= off and off + len <= hi, by off, then by len; record = the delimiters in front of off
    std::vector<BzmHit> naive(const uint8_t *text, uint64_t n, uint64_t lo, uint64_t hi, bool records, uint32_t delim) const
    {
        std::vector<BzmHit> v;
        hi = std::min(hi, n);
        uint64_t rec = 0;
        for (uint64_t o = 0; o < hi; o++) {
            if (o >= lo)
                for (auto &d : distinct)
                    if (at(text, o, hi, d.first)) v.push_back(BzmHit{o, records ? rec : 0, d.second, (uint32_t)d.first.size()});
            rec += text[o] == delim;
        }
        return v;
    }
};

// ---- (a) the compile ------------------------------------------------------------------------------------------------------------
static Bytes B(const char *s) { return Bytes(s, s + strlen(s)); }
// the table walked as the matcher walks it, without a tile: the hits at text[o ..) bounded by lim
static std::vector<std::pair<uint32_t, uint32_t>> table_walk(const Set &s, const uint8_t *text, uint64_t o, uint64_t lim)
{
    std::vector<std::pair<uint32_t, uint32_t>> v; // (pattern, len)
    uint32_t st = 0;
    for (uint32_t depth = 0; o + depth < lim && depth < s.plan.max_len; depth++) {
        const size_t at = (size_t)st * s.plan.classes + s.cls[text[o + depth]];
        CHECK(at < s.plan.table.size(), "the walk leaves the table");
        st = s.table[at];
        if (!st) break;
        CHECK(st < s.plan.states, "state %u of %u", st, s.plan.states);
        if (st <= s.plan.distinct) v.push_back({s.pat_no[st - 1], depth + 1});
    }
    return v;
}
static void compile_case(const Pats &pats, unsigned flags, const Bytes &text, uint64_t want_distinct, const char *what)
{
    const Set s(pats, flags);
    CHECK(s.ok, "%s: %s", what, s.why.c_str());
    CHECK(s.plan.patterns == pats.size() && s.plan.distinct == want_distinct && s.distinct.size() == want_distinct, "%s: %llu distinct, want %llu", what,
          (ull)s.plan.distinct, (ull)want_distinct);
    CHECK(s.plan.table.size() == (size_t)s.plan.states * s.plan.classes && s.plan.classes <= 256 && s.plan.states <= 65536, "%s: the table", what);
    uint32_t mn = ~0u, mx = 0;
    for (auto &p : pats) mn = std::min<uint32_t>(mn, p.size()), mx = std::max<uint32_t>(mx, p.size());
    CHECK(s.plan.min_len == mn && s.plan.max_len == mx, "%s: lengths", what);
    for (uint32_t b = 0; b < 256; b++) CHECK(s.cls[b] < s.plan.classes && s.first[b] == s.table[s.cls[b]], "%s: class of byte %u", what, b);
    const Text t(text.data(), text.size());
    for (uint64_t lim : {(uint64_t)text.size(), (uint64_t)text.size() / 2})
        for (uint64_t o = 0; o < lim; o++) {
            const auto got = table_walk(s, t.p, o, lim);
            size_t k = 0;
            for (auto &d : s.distinct)
                if (s.at(t.p, o, lim, d.first)) {
                    CHECK(k < got.size() && got[k].first == d.second && got[k].second == d.first.size(), "%s: at %llu the walk misses pattern %u", what,
                          (ull)o, d.second);
                    k++;
                }
            CHECK(k == got.size(), "%s: at %llu the walk finds %zu, the truth %zu", what, (ull)o, got.size(), k);
        }
}
static void refused(const Pats &pats, unsigned flags, const char *needle)
{
    const Set s(pats, flags);
    CHECK(!s.ok && s.why.find(needle) != std::string::npos, "refused with \"%s\", want \"%s\"", s.why.c_str(), needle);
}
static void part_compile()
{
    Bytes text;
    for (int i = 0; i < 3000; i++) text.push_back("abcABC@`[{xyz\xC0\xE0 "[below(16)]);
    compile_case({B("abc"), B("abc"), B("b"), B("abc")}, 0, text, 2, "duplicates");
    compile_case({B("Abc"), B("aBC"), B("abc"), B("B")}, BZM_FOLD_ASCII, text, 2, "duplicates by folding");
    compile_case({B("Abc"), B("aBC"), B("abc"), B("B")}, 0, text, 4, "no duplicates without folding");
    compile_case({B("ab"), B("abc"), B("a"), B("abca")}, 0, text, 4, "prefixes");
    compile_case({B("bc"), B("abc"), B("c"), B("cabc")}, BZM_FOLD_ASCII, text, 4, "suffixes");
    compile_case({B("@a"), B("`a"), B("[b"), B("{b"), B("\xC0"), B("\xE0z"), B("Z{")}, BZM_FOLD_ASCII, text, 7, "neighbours that do not fold");
    {
        const Set s({B("@"), B("["), B("\xC0"), B("Q")}, BZM_FOLD_ASCII);
        CHECK(s.ok && s.cls['@'] != s.cls['`'] && s.cls['['] != s.cls['{'] && s.cls[0xC0] != s.cls[0xE0] && s.cls['Q'] == s.cls['q'] && s.cls['q'] != 0,
              "what folds");
        CHECK(s.cls['`'] == 0 && s.cls['{'] == 0 && s.cls[0xE0] == 0 && s.plan.classes == 5, "the dead class");
    }
    {
        Pats all;
        Bytes every;
        for (uint32_t b = 0; b < 256; b++) all.push_back(Bytes(1, (uint8_t)b)), every.push_back((uint8_t)b);
        for (int i = 0; i < 500; i++) every.push_back((uint8_t)below(256));
        compile_case(all, 0, every, 256, "every byte value");
        const Set s(all, 0);
        CHECK(s.plan.classes == 256 && s.plan.states == 257, "256 classes");
        compile_case(all, BZM_FOLD_ASCII, every, 230, "every byte value, folded");
    }
    {   // 257 patterns of 255 bytes that share nothing: 65,535 states; one byte more: refused
        Pats big;
        for (uint32_t i = 0; i < 257; i++) {
            Bytes p(255, (uint8_t)(i & 0xFF));
            if (i == 256) p.assign(255, 0), p[0] = 1, p[1] = 7; // shares its first byte with pattern 1: 254 new states
            big.push_back(p);
        }
        big.push_back(B("\x02")); // (a prefix: no new state)
        big.push_back(Bytes{9, 8}); // shares a byte with pattern 9: 1 new state
        const Set s(big, 0);
        CHECK(s.ok && s.plan.states == 65536, "65,535 states beyond the root are accepted: %s, %u", s.why.c_str(), s.plan.states);
        Bytes t(600, 9);
        t[300] = 1, t[301] = 7;
        compile_case(big, 0, t, 259, "the largest trie");
        big.push_back(Bytes{9, 7});
        refused(big, 0, "65536 states");
    }
    refused({}, 0, "0 patterns");
    refused({B("a"), Bytes()}, 0, "pattern 1 has 0 bytes");
    refused({B("a"), B("b"), Bytes(257, 'x')}, 0, "pattern 2 has 257 bytes");
    refused({B("a")}, 2, "flags 0x2");
    char err[100];
    BzmPlan plan;
    CHECK(!bzm_compile(nullptr, nullptr, 1, 0, plan, err, sizeof err) && strstr(err, "null"), "a null array");
    printf("compile: held\n");
}

// ---- (b) the device: scan_host.h's model with BzmMatcher --------------------------------------------------------------------------
static GrepTruth grep_naive(const Bytes &text, const Set &s, uint32_t delim, uint32_t invert)
{
    GrepTruth tr;
    const uint64_t n = text.size();
    uint64_t start = 0, rec = 0;
    auto close = [&](uint64_t end) {
        bool hit = false;
        for (uint64_t o = start; o < end && !hit; o++) hit = s.any_at(text.data(), o, n);
        if (hit != (invert != 0)) {
            tr.ent.push_back(BzgEntry{rec, start, end - start, tr.out.size()});
            tr.out.insert(tr.out.end(), text.begin() + start, text.begin() + end);
        }
        rec++, start = end;
    };
    for (uint64_t i = 0; i < n; i++)
        if (text[i] == delim) close(i + 1);
    if (start < n) close(n);
    tr.nrecords = rec;
    return tr;
}
// one grep call; blocks: the windows' new bytes (empty: the raw call)
static void grep_set(const Bytes &text, const Set &set, uint32_t delim, uint32_t invert, const std::vector<uint64_t> &blocks, int out_kind, int ent_kind)
{
    grep_call(text, grep_naive(text, set, delim, invert), [&](const BzgWindow &w) { return set.matcher(delim, w.n); }, set.plan.max_len, invert,
              (uint8_t)(delim == 0xEE ? 0xED : 0xEE), blocks, out_kind, ent_kind);
}

// one raw search call with `max` hit slots; returns the hits
static uint64_t search_raw(const Bytes &src, const Set &set, uint32_t delim, bool records, uint64_t max)
{
    const uint64_t n = src.size();
    const Text text(src.data(), n);
    BzmSetWalk walk;
    walk.begin(set.plan.max_len, 0, max, 0, n, 0, 0);
    uint64_t lim = 0, hits, delims;
    const BzfWindow w = walk.window_set(n, true, &lim);
    CHECK(lim == n || w.s_hi == w.s_lo, "the raw window ends at the text's end");
    std::vector<BzmHit> out;
    search_run(text.p, w, set.matcher(delim, lim), records, walk, out, &hits, &delims);
    same_hits(out, set.naive(text.p, n, 0, n, records, delim), hits, max, "raw", n);
    CHECK(!records || delims == (uint64_t)std::count(text.p, text.p + n, (uint8_t)delim), "raw (%llu): delimiters", (ull)n);
    return hits;
}

static Bytes word(uint32_t len, const char *alphabet)
{
    Bytes p(len);
    const size_t a = strlen(alphabet);
    for (auto &b : p) b = (uint8_t)alphabet[below(a)];
    return p;
}
static void plant(Bytes &text, uint64_t at, const Bytes &p)
{
    if (at + p.size() <= text.size()) memcpy(&text[at], p.data(), p.size());
}

static void part_matcher()
{
    const uint64_t ns[] = {0, 1, 15, 16, 17, 4095, 4096, 4097, 8192, 12289};
    static const uint32_t lens[] = {1, 2, 4, 5, 17, 255, 256};
    uint64_t cases = 0, found = 0;
    for (uint64_t n : ns)
        for (unsigned fold = 0; fold < 2; fold++) {
            // a chain: every length a prefix of the next (short and long at the same start), and seeded words of every length
            Pats pats;
            const Bytes longest = word(256, fold ? "aBcD" : "abcd");
            for (uint32_t l : lens) pats.push_back(Bytes(longest.begin(), longest.begin() + l));
            for (uint32_t l : lens) pats.push_back(word(l, "abcd"));
            pats.push_back(B("\n")), pats.push_back(B("b\n")), pats.push_back(pats[3]);
            const Set set(pats, fold ? (unsigned)BZM_FOLD_ASCII : 0u);
            CHECK(set.ok, "%s", set.why.c_str());
            // seeded text over the letters and the delimiter
            Bytes text(n);
            for (auto &c : text) c = (uint8_t)"abcdABCD\nx"[below(10)];
            found += search_raw(text, set, '\n', true, ~0ull), cases++;
            grep_set(text, set, '\n', 0, {}, 2, 2), grep_set(text, set, '\n', 1, {}, 2, 2);
            // the fixed places: offset 0, ending at byte n - 1, across a thread edge, a wave edge, a tile edge -- every length there, the
            // chain's patterns at one start; the longest cut by the text's end while its prefixes still match
            for (uint32_t l : lens) {
                Bytes t2(n, 'x');
                const Bytes p(longest.begin(), longest.begin() + l);
                uint64_t planted = 0, last_end = 0;
                std::vector<uint64_t> es{0, n - l, (uint64_t)16 - l / 2, (uint64_t)1024 - l / 2, (uint64_t)4096 - l / 2, 4095, (uint64_t)8192 - l + 1};
                std::sort(es.begin(), es.end());
                for (uint64_t e : es)
                    if (e < n && e + l <= n && (planted == 0 || e >= last_end)) plant(t2, e, p), planted++, last_end = e + l;
                if (n > 3) // (the longest, cut by the text's end)
                    for (uint64_t at = n - std::min<uint64_t>(n, 1 + below(l)), j = 0; at + j < n; j++) t2[at + j] = longest[j];
                for (uint64_t at = 40; at < n; at += 1000) t2[at] = '\n';
                const uint64_t h = search_raw(t2, set, '\n', true, ~0ull);
                CHECK(h >= planted, "planted %llu, found %llu", (ull)planted, (ull)h);
                found += h, cases++;
                grep_set(t2, set, '\n', 0, {}, 2, 2), grep_set(t2, set, '\n', 1, {}, 1, 0);
            }
            // one byte value everywhere, the set every run of it up to 256: every slot, three, none; the delimiter a pattern byte
            {
                Pats runs;
                for (uint32_t l : lens) runs.push_back(Bytes(l, 'z'));
                const Set rs(runs, fold ? (unsigned)BZM_FOLD_ASCII : 0u);
                const Bytes t3(n, fold ? 'Z' : 'z');
                uint64_t want = 0;
                for (uint32_t l : lens) want += n >= l ? n - l + 1 : 0;
                CHECK(search_raw(t3, rs, fold ? 'Z' : 'z', true, ~0ull) == want, "a buffer of one byte value");
                CHECK(search_raw(t3, rs, 'z', true, 3) == want, "a buffer of one byte value, three slots");
                CHECK(search_raw(t3, rs, 'z', false, 0) == want, "a buffer of one byte value, no slots");
                grep_set(t3, rs, fold ? 'Z' : 'z', 0, {}, 2, 2);
                grep_set(t3, rs, 'q', 0, {}, 2, 2), grep_set(t3, rs, 'q', 1, {}, 3, 3);
                cases += 3;
            }
        }
    printf("matcher: %llu search cases held, %llu hits\n", (ull)cases, (ull)found);
}

// ---- (c) windows -----------------------------------------------------------------------------------------------------------------------
static void part_windows(uint64_t cases)
{
    uint64_t windows = 0, finished = 0, cut = 0;
    for (uint64_t c = 0; c < cases; c++) {
        const size_t nb = 1 + below(7);
        std::vector<uint64_t> blk(nb);
        uint64_t total = 0;
        for (auto &e : blk) e = below(3) ? 1 + below(300) : 1 + below(9000), total += e;
        // the set: a short pattern and a long one that begins with it, and a few words; sometimes a pattern holds the delimiter
        const unsigned fold = (unsigned)below(2);
        const uint32_t ls = 1 + (uint32_t)below(4), ll = below(3) ? ls + 1 + (uint32_t)below(8) : 2 + (uint32_t)below(255);
        const Bytes lng = word(ll, below(4) ? "ab" : "aB\n"), sht(lng.begin(), lng.begin() + std::min(ls, ll - 1));
        Pats pats{lng, sht};
        for (uint64_t k = below(4); k > 0; k--) pats.push_back(word(1 + (uint32_t)below(below(2) ? 5 : 40), "abAB"));
        const Set set(pats, fold ? (unsigned)BZM_FOLD_ASCII : 0u);
        CHECK(set.ok, "%s", set.why.c_str());
        const bool records = below(4) != 0;
        Bytes truth(total);
        for (auto &ch : truth) ch = (uint8_t)"abAx\n"[below(below(3) ? 5 : 4)];
        // on every block edge: the short pattern ending in front of it and the long one at the same start spanning it; delimiters
        uint64_t edge = 0;
        std::vector<uint64_t> wins;
        for (size_t k = 0; k < nb; k++) {
            edge += blk[k];
            if (below(4)) plant(truth, edge - std::min<uint64_t>(edge, sht.size() + below(ll - sht.size() + 1)), lng);
            if (edge < total && below(2)) truth[edge - below(2)] = '\n';
        }
        // a range of whole blocks from `first` on, its ends anywhere: they cut matches at either end
        const size_t first = below(nb), last = first + 1 + below(nb - first);
        uint64_t start = 0, stop = 0;
        for (size_t k = 0; k < last; k++) (k < first ? start : stop) += blk[k];
        stop += start;
        const uint64_t lo = below(2) ? start : start + below(stop - start), hi = below(2) ? stop : lo + below(stop - lo + 1);
        const std::vector<BzmHit> want = set.naive(truth.data(), total, lo, hi, records, '\n');
        for (uint64_t o = lo; o < hi && hi < total; o++) cut += set.at(truth.data(), o, total, lng) && !set.at(truth.data(), o, hi, lng) && set.at(truth.data(), o, hi, sht);
        const uint64_t maxes[] = {~0ull, want.size(), want.size() ? want.size() - 1 : 0, 0, below(want.size() + 2)};
        const uint64_t max = maxes[below(5)];
        const uint64_t room = below(3) ? 1 + below(600) : 1 + below(20000);
        const size_t bmax = 1 + below(4);
        uint64_t rec_start = 0;
        for (uint64_t i = 0; i < start; i++) rec_start += truth[i] == '\n';
        BzmSetWalk walk;
        walk.begin(set.plan.max_len, BZF_FRONT, max, lo, hi, start, records ? rec_start : 0);
        ZeroLookTwin zero; // (no assertion is the zero case)
        zero.begin(set.plan.max_len, BZF_FRONT, max, lo, hi, start, records ? rec_start : 0);
        std::vector<BzmHit> got((size_t)std::min<uint64_t>(max, want.size() + 8), BzmHit{~0ull, ~0ull, ~0u, ~0u});
        Bytes carry;
        uint64_t at_out = start;
        auto run = [&](const uint8_t *d, const BzfWindow &w, uint64_t lim, uint64_t bytes, bool is_last) {
            CHECK(w.s_lo <= w.s_hi && w.s_hi <= lim && lim <= w.n, "window: starts [%llu, %llu) lim %llu n %llu", (ull)w.s_lo, (ull)w.s_hi, (ull)lim, (ull)w.n);
            zero.window(walk, bytes, is_last, w, lim);
            std::vector<BzmHit> out;
            uint64_t hits, delims;
            search_run(d, w, set.matcher('\n', lim), records, walk, out, &hits, &delims);
            for (size_t i = 0; i < out.size(); i++) got.at((size_t)walk.rank + i) = out[i];
            walk.advance_set(bytes, hits, delims, is_last);
            zero.advance(walk, bytes, hits, delims, is_last);
            windows++;
        };
        for (size_t at = first; at < last;) {
            uint64_t bytes = 0;
            size_t nbw = 0;
            while (at + nbw < last && nbw < bmax && (nbw == 0 || bytes + blk[at + nbw] <= room)) bytes += blk[at + nbw], nbw++;
            if (at == first) wins.clear();
            wins.push_back(bytes);
            // SearchSink::room and ::window: a staging buffer of exactly these bytes, the carry in front of the window
            const Text staging(BZF_FRONT + bytes);
            memset(staging.p, poison_front, BZF_FRONT);
            CHECK(carry.size() == walk.carry, "the carry");
            if (!carry.empty()) memcpy(staging.p + BZF_FRONT - carry.size(), carry.data(), carry.size());
            memcpy(staging.p + BZF_FRONT, &truth[at_out], (size_t)bytes);
            uint64_t lim = 0;
            const BzfWindow w = walk.window_set(bytes, false, &lim);
            const uint64_t keep = walk.carry_after_set(bytes);
            const Bytes next(staging.p + w.n - keep, staging.p + w.n);
            run(staging.p, w, lim, bytes, false);
            carry = next;
            at_out += bytes, at += nbw;
        }
        if (walk.carry) { // SearchSink::finish: the carry is the text
            const Text held(carry.data(), carry.size());
            walk.front = walk.carry;
            uint64_t lim = 0;
            const BzfWindow w = walk.window_set(0, true, &lim);
            run(held.p, w, lim, 0, true);
            finished++;
        }
        same_hits(got, want, walk.rank, max, "windows", c);
        // the grep over the same windows (it takes the whole text of the blocks it is given)
        const Bytes part(truth.begin() + start, truth.begin() + stop);
        grep_set(part, set, '\n', (uint32_t)below(2), wins, (int)below(5), (int)below(5));
    }
    CHECK(finished > cases / 4 && cut > 0, "the cases reach the edges: %llu finishing windows, %llu long patterns cut by the range", (ull)finished, (ull)cut);
    printf("windows: %llu cases held, %llu windows, %llu finishing ones, %llu cut by the range\n", (ull)cases, (ull)windows, (ull)finished, (ull)cut);
}

int main(int argc, char **argv)
{
    rng_state = argc > 1 ? strtoull(argv[1], nullptr, 10) * 0x9E3779B97F4A7C15ull + 1 : 1;
    const uint64_t cases = argc > 2 ? strtoull(argv[2], nullptr, 10) : 200;
    part_compile();
    part_matcher();
    part_windows(cases);
    return 0;
}
