// regex_host.cpp -- regular expressions for search and grep without a device, built with g++ -fsanitize=address,undefined.
// (a) The compile of banzai_amd/csrc/regex_plan.h against a naive matcher over the harness's OWN expressions: seeded random trees of
//     the grammar, printed for the compiler and matched here on the tree, at every offset of seeded texts, with two bounds and two
//     spans; every refused form; the state bound; the blow-up; what folds and what does not.
// (b) The matchers of banzai_amd/csrc/regex_core.h -- BzrMatcher<true, false> and BzrMatcher<false, false>, the kernels' own text -- thread by
//     thread and tile by tile in the kernels' layout over a model of the LDS: both passes of search_tiles and the scan between them,
//     both passes of grep_tiles with grep_core.h's phases and scan.  The table, the LDS model and every buffer have their exact sizes.
// (c) The windows: BzmSetWalk (search_plan.h) and BzgWalk (grep_plan.h) with (b) as the device, against brute force per byte.
//
//   regex_host <seed> <cases>                          exit status 0: everything held
//   regex_host hits EXPRFILE TEXTFILE FLAGS SPAN       one expression a line; prints "off pattern len" for every hit of the text
#define HOST_NAME "regex_host"
#include <bitset>
#include <set>
#include <string>

#include "../../include/bzhip.h"
#include "../../banzai_amd/csrc/regex_core.h"
#include "../../banzai_amd/csrc/regex_plan.h"
#include "regex_ex_host.h"
#include "scan_host.h"

typedef std::vector<Bytes> Pats;

static_assert(sizeof(bzh_set_hit) == sizeof(BzmHit) && sizeof(BzmHit) == 24, "a set's hit is three words");
static_assert(sizeof(bzh_grep_entry) == sizeof(BzgEntry), "an entry is four words");
static_assert(sizeof(bzh_regex_info) == 40, "bzh_regex_info");
static_assert((uint32_t)BZR_LDS_ROWS == (uint32_t)BZR_LDS_ENTRIES, "one bound");

static Bytes B(const char *s) { return Bytes(s, s + strlen(s)); }

// ---- the harness's own expressions: a tree, its text for the compiler, and the naive matcher on the tree --------------------------
static const char ALPHA[] = "abAB01 _\n-z";
static Ex lit(uint8_t b)
{
    Ex e;
    e.set[b] = true;
    char q[8];
    if (strchr("\\.[]()|*+?{}^$-/", b)) snprintf(q, sizeof q, "\\%c", b), e.text = q;
    else if (b == '\n') e.text = below(2) ? "\\n" : "\\x0a";
    else if (b < 32 || b >= 127) snprintf(q, sizeof q, "\\x%02X", b), e.text = q;
    else e.text = std::string(1, (char)b);
    return e;
}
static void add_class(Ex &e, char c) // \d \w \s and their complements, into e.set
{
    std::bitset<256> s;
    const char l = (char)(c | 32);
    for (uint32_t b = 0; b < 256; b++)
        s[b] = l == 'd' ? (b >= '0' && b <= '9') : l == 'w' ? ((b >= '0' && b <= '9') || (b >= 'a' && b <= 'z') || (b >= 'A' && b <= 'Z') || b == '_') : (b == ' ' || (b >= 9 && b <= 13));
    if (c < 'a') s = ~s;
    e.set |= s;
}
static Ex random_set(bool dotall)
{
    Ex e;
    const uint64_t k = below(10);
    if (k < 5) return lit((uint8_t)ALPHA[below(sizeof ALPHA - 1)]);
    if (k == 5) {
        for (uint32_t b = 0; b < 256; b++) e.set[b] = dotall || b != '\n';
        e.text = ".";
        return e;
    }
    if (k == 6) {
        const char c = "dDwWsS"[below(6)];
        add_class(e, c);
        e.text = std::string("\\") + c;
        return e;
    }
    e.neg = below(3) == 0;
    e.text = e.neg ? "[^" : "[";
    for (uint64_t items = 1 + below(3); items > 0; items--) {
        const uint64_t w = below(4);
        if (w == 0) {
            const char c = "dws"[below(3)];
            add_class(e, c);
            e.text += std::string("\\") + c;
        } else if (w == 1) {
            static const char *const ranges[] = {"a-b", "A-Z", "0-1", "@-Z", "a-z", "\\x00-\\x20", "Y-b"};
            static const uint8_t lo[] = {'a', 'A', '0', '@', 'a', 0, 'Y'}, hi[] = {'b', 'Z', '1', 'Z', 'z', 0x20, 'b'};
            const uint64_t r = below(7);
            for (uint32_t b = lo[r]; b <= hi[r]; b++) e.set[b] = true;
            e.text += ranges[r];
        } else {
            const uint8_t b = (uint8_t)ALPHA[below(sizeof ALPHA - 1)];
            e.set[b] = true;
            e.text += b == '-' ? "\\-" : b == '\n' ? "\\n" : std::string(1, (char)b);
        }
    }
    e.text += "]";
    return e;
}
static Ex random_ex(uint32_t depth, bool dotall)
{
    const uint64_t k = depth == 0 ? 0 : below(8);
    Ex e;
    if (k < 2) return random_set(dotall);
    if (k < 5) {
        e.kind = Ex::CAT;
        for (uint64_t n = 2 + below(3); n > 0; n--) e.kids.push_back(random_ex(depth - 1, dotall));
    } else if (k == 5) {
        e.kind = Ex::ALT;
        for (uint64_t n = 2 + below(2); n > 0; n--) e.kids.push_back(random_ex(depth - 1, dotall));
    } else {
        e.kind = Ex::REP;
        e.kids.push_back(random_ex(depth - 1, dotall));
        static const uint32_t los[] = {0, 0, 1, 2, 0, 1, 3, 2}, his[] = {1, ~0u, ~0u, 2, 3, 2, ~0u, 5};
        const uint64_t r = below(8);
        e.lo = los[r], e.hi = his[r];
    }
    return e;
}

// ---- a compiled automaton as the device holds it --------------------------------------------------------------------------------------
struct Auto {
    BzrPlan plan;
    uint8_t *cls = nullptr;
    uint16_t *first = nullptr, *table = nullptr;
    uint32_t *pat_no = nullptr;
    bool ok = false;
    std::string why;
    Auto(const Pats &exprs, unsigned flags, uint32_t span)
    {
        std::vector<const uint8_t *> ptr;
        std::vector<size_t> len;
        for (const Bytes &p : exprs) ptr.push_back(p.data()), len.push_back(p.size());
        char err[200] = "";
        ok = bzr_compile(ptr.data(), len.data(), exprs.size(), flags, span, plan, err, sizeof err);
        why = err;
        if (!ok) return;
        cls = exact(plan.cls, 256), first = exact(plan.first, 256);
        table = exact(plan.table.data(), plan.table.size()), pat_no = exact(plan.pat_no.data(), plan.pat_no.size());
    }
    ~Auto() { free(cls), free(first), free(table), free(pat_no); }
    Auto(const Auto &) = delete;
    template <bool L>
    BzrMatcher<L, false> matcher(uint32_t delim, uint64_t lim) const
    {
        return BzrMatcher<L, false>{{BzrAuto{BzmSet{cls, first, table, pat_no, plan.classes, plan.nterm, plan.max_len, delim, lim}, plan.states * plan.classes}}, {}};
    }
    // the table walked without a tile, every invariant checked on the way: the hit at text[o ..) bounded by lim
    bool walk(const uint8_t *text, uint64_t o, uint64_t lim, uint32_t *pattern, uint32_t *len) const
    {
        uint32_t st = 0;
        bool hit = false;
        for (uint32_t depth = 0; o + depth < lim && depth < plan.max_len; depth++) {
            const size_t at = (size_t)st * plan.classes + cls[text[o + depth]];
            CHECK(at < plan.table.size(), "the walk leaves the table");
            st = table[at];
            if (!st) break;
            CHECK(st < plan.states, "state %u of %u", st, plan.states);
            if (st <= plan.nterm) hit = true, *pattern = pat_no[st - 1], *len = depth + 1;
        }
        return hit;
    }
    // THE RULE by the table (the table itself is held to the tree and to Python's re elsewhere): every hit with lo <= off and
    // off + len <= hi
    std::vector<BzmHit> naive(const uint8_t *text, uint64_t n, uint64_t lo, uint64_t hi, bool records, uint32_t delim) const
    {
        std::vector<BzmHit> v;
        hi = std::min(hi, n);
        uint64_t rec = 0;
        for (uint64_t o = 0; o < hi; o++) {
            uint32_t pat, len;
            if (o >= lo && walk(text, o, hi, &pat, &len)) v.push_back(BzmHit{o, records ? rec : 0, pat, len});
            rec += text[o] == delim;
        }
        return v;
    }
    bool any_at(const uint8_t *text, uint64_t o, uint64_t lim) const
    {
        uint32_t pat, len;
        return walk(text, o, lim, &pat, &len);
    }
};

// ---- (a) the compile -----------------------------------------------------------------------------------------------------------------
static void table_invariants(const Auto &a, const char *what)
{
    const BzrPlan &p = a.plan;
    CHECK(p.table.size() == (size_t)p.states * p.classes && p.classes >= 1 && p.classes <= 256 && p.states >= 2 && p.states <= 65536, "%s: the table", what);
    CHECK(p.nterm >= 1 && p.nterm < p.states && p.pat_no.size() == p.nterm, "%s: the terminals", what);
    for (uint32_t b = 0; b < 256; b++) CHECK(a.cls[b] < p.classes && a.first[b] == a.table[a.cls[b]], "%s: class of byte %u", what, b);
    std::vector<uint32_t> seen(p.states, 0), order{0};
    seen[0] = 1;
    uint32_t next_term = 1, next_rest = p.nterm + 1;
    for (size_t h = 0; h < order.size(); h++)
        for (uint32_t c = 0; c < p.classes; c++) {
            const uint32_t t = a.table[(size_t)order[h] * p.classes + c];
            CHECK(t < p.states, "%s: an entry names a row", what);
            if (!t || seen[t]) continue;
            seen[t] = 1, order.push_back(t);
            if (t <= p.nterm) CHECK(t == next_term++, "%s: terminal rows in breadth-first order", what);
            else CHECK(t == next_rest++, "%s: rows in breadth-first order", what);
        }
    CHECK(order.size() == p.states, "%s: every row is reached", what);
    CHECK(p.min_len >= 1 && p.min_len <= p.max_len && p.max_len <= p.max_span, "%s: lengths %u..%u", what, p.min_len, p.max_len);
}
static void refused(const char *expr, unsigned flags, uint32_t span, const char *needle)
{
    const Auto a({B(expr)}, flags, span);
    CHECK(!a.ok && a.why.find(needle) != std::string::npos && a.why.find("expression 0, byte ") != std::string::npos, "\"%s\" refused with \"%s\", want \"%s\"", expr,
          a.why.c_str(), needle);
}
static void info_case(const char *expr, unsigned flags, uint32_t span, uint32_t mn, uint32_t mx, uint32_t unb)
{
    const Auto a({B(expr)}, flags, span);
    CHECK(a.ok, "%s: %s", expr, a.why.c_str());
    table_invariants(a, expr);
    CHECK(a.plan.min_len == mn && a.plan.max_len == mx && a.plan.unbounded == unb, "%s: %u..%u unbounded %u, want %u..%u %u", expr, a.plan.min_len, a.plan.max_len,
          a.plan.unbounded, mn, mx, unb);
}
static void part_compile(uint64_t cases)
{
    // seeded trees against the tree matcher
    uint64_t checked = 0, live = 0, refused_big = 0;
    for (uint64_t c = 0; c < cases; c++) {
        const unsigned flags = (unsigned)below(4); // fold, dotall
        const bool fold = flags & BZR_FOLD_ASCII, dotall = (flags & BZR_DOTALL) != 0;
        std::vector<Ex> exs;
        Pats exprs;
        for (uint64_t k = 1 + below(3); k > 0; k--) {
            Ex e = random_ex(1 + (uint32_t)below(3), dotall);
            while (min_len(e) == 0 || min_len(e) > 5) e = random_ex(1 + (uint32_t)below(3), dotall);
            const std::string s = print(e, true);
            exs.push_back(e), exprs.push_back(Bytes(s.begin(), s.end()));
        }
        Bytes text(100 + below(100));
        for (auto &ch : text) ch = below(12) ? (uint8_t)ALPHA[below(sizeof ALPHA - 1)] : (uint8_t)below(256);
        const Text t(text.data(), text.size());
        for (uint32_t span : {256u, 5u}) {
            const Auto a(exprs, flags, span);
            if (!a.ok) { // (only the bounds may refuse what the grammar made)
                CHECK(a.why.find("states") != std::string::npos || a.why.find("positions") != std::string::npos, "case %llu: %s", (ull)c, a.why.c_str());
                refused_big++;
                continue;
            }
            table_invariants(a, "a seeded case");
            bool longer = false;
            for (uint64_t lim : {(uint64_t)text.size(), (uint64_t)text.size() / 2})
                for (uint64_t o = 0; o < lim; o++) {
                    uint64_t best = 0;
                    uint32_t who = 0;
                    for (uint32_t j = 0; j < exs.size(); j++) {
                        const Ends en = ends(exs[j], t.p, text.size(), lim, Ends{o}, fold);
                        for (uint64_t e : en) {
                            if (e - o > span) longer = true;
                            else if (e > o && e - o > best) best = e - o, who = j;
                        }
                    }
                    uint32_t pat = 0, len = 0;
                    const bool hit = a.walk(t.p, o, lim, &pat, &len);
                    CHECK(hit == (best > 0) && (!hit || (len == best && pat == who)), "case %llu (%s ...) flags %u span %u at %llu: the table says %d (%u, %u), the tree (%u, %llu)",
                          (ull)c, (const char *)std::string(exprs[0].begin(), exprs[0].end()).c_str(), flags, span, (ull)o, (int)hit, pat, len, who, (ull)best);
                    checked++, live += hit;
                }
            CHECK(!longer || a.plan.unbounded, "case %llu: a match above the span, and unbounded is 0", (ull)c);
        }
    }
    CHECK(live > checked / 50, "the seeded cases match somewhere: %llu of %llu", (ull)live, (ull)checked);

    // the figures
    info_case("abc", 0, 0, 3, 3, 0);
    info_case("a+", 0, 0, 1, 256, 1);
    info_case("a{3}", 0, 3, 3, 3, 0);
    info_case("a{2,256}", 0, 0, 2, 256, 0);
    info_case("a{2,256}b", 0, 0, 3, 256, 1);
    info_case("(abc)+|a{2,3}", 0, 16, 2, 16, 1);
    info_case("err(or)?", BZR_FOLD_ASCII, 0, 3, 5, 0);
    info_case("(?:GET|POST) /", 0, 0, 5, 6, 0);
    info_case("(ab)*c", 0, 0, 1, 256, 1); // (the start subset recurs behind "ab": a row of its own, checked by table_invariants)
    info_case("[^\\x00-\\xff]|a", 0, 0, 1, 1, 0);
    info_case("\\x41\\0\\/\\-\\n\\t\\r\\f\\v\\\\\\.\\[\\]\\(\\)\\|\\*\\+\\?\\{\\}\\^\\$", 0, 0, 23, 23, 0);
    info_case("[]a]{2}[a\\]-]}]", 0, 0, 5, 5, 0);
    // every refused form
    refused("^a", 0, 0, "anchors");
    refused("a$", 0, 0, "anchors");
    refused("a\\b", 0, 0, "\\b");
    refused("(a)\\1", 0, 0, "backreferences");
    refused("a(?=b)", 0, 0, "lookaround");
    refused("a(?!b)", 0, 0, "lookaround");
    refused("(?<=a)b", 0, 0, "lookaround");
    refused("(?P<n>a)", 0, 0, "named groups");
    refused("(?i)a", 0, 0, "inline flags");
    refused("a*?", 0, 0, "lazy");
    refused("a+?", 0, 0, "lazy");
    refused("a??", 0, 0, "lazy");
    refused("a{2}?", 0, 0, "lazy");
    refused("a*+", 0, 0, "possessive");
    refused("a**", 0, 0, "quantifier");
    refused("*a", 0, 0, "nothing to repeat");
    refused("a{", 0, 0, "well-formed bound");
    refused("a{x}", 0, 0, "well-formed bound");
    refused("a{,3}", 0, 0, "well-formed bound");
    refused("a{2", 0, 0, "well-formed bound");
    refused("{2}", 0, 0, "well-formed bound");
    refused("a{257}", 0, 0, "bound above 256");
    refused("a{1,257}", 0, 0, "bound above 256");
    refused("a{3,2}", 0, 0, "below its minimum");
    refused("[abc", 0, 0, "unbalanced bracket");
    refused("[]", 0, 0, "unbalanced bracket");
    refused("(ab", 0, 0, "unbalanced bracket");
    refused("ab)", 0, 0, "unbalanced bracket");
    refused("[b-a]", 0, 0, "in front of its start");
    refused("a\\", 0, 0, "backslash");
    refused("\\q", 0, 0, "escape");
    refused("\\x4", 0, 0, "hexadecimal");
    refused("a*", 0, 0, "empty string");
    refused("a?b*", 0, 0, "empty string");
    refused("(a|)", 0, 0, "empty string");
    refused("a{0}", 0, 0, "empty string");
    refused("a{3}", 0, 2, "max_span 2");
    refused("[^\\x00-\\xff]", 0, 0, "max_span");
    {
        const Auto a({B("ab"), B("c*")}, 0, 0);
        CHECK(!a.ok && a.why.find("expression 1, byte 0") != std::string::npos, "the second expression is named: %s", a.why.c_str());
        const Auto b({B("ab"), B("cd(")}, 0, 0);
        CHECK(!b.ok && b.why.find("expression 1, byte 2") != std::string::npos, "the byte is named: %s", b.why.c_str());
        const Auto c({}, 0, 0), d({B("a"), Bytes()}, 0, 0), e({Bytes(4097, 'a')}, 0, 0), f({B("a")}, 8, 0), g({B("a")}, 0, 257);
        CHECK(!c.ok && !d.ok && !e.ok && !f.ok && !g.ok, "count 0, an empty expression, 4,097 bytes, an undefined flag, a span above 256");
        const Auto h({Bytes(4096, 'a')}, 0, 0);
        CHECK(!h.ok && h.why.find("max_span") != std::string::npos, "4,096 literal bytes parse, and exceed the span: %s", h.why.c_str());
        BzrPlan plan;
        char err[100];
        CHECK(!bzr_compile(nullptr, nullptr, 1, 0, 0, plan, err, sizeof err) && strstr(err, "null"), "a null array");
    }
    // what folds and what does not
    {
        const Auto a({B("@"), B("\\["), B("\xC0"), B("Q"), B("[x-z]")}, BZR_FOLD_ASCII, 0);
        CHECK(a.ok && a.cls['@'] != a.cls['`'] && a.cls['['] != a.cls['{'] && a.cls[0xC0] != a.cls[0xE0] && a.cls['Q'] == a.cls['q'] && a.cls['q'] != 0 &&
                  a.cls['Y'] == a.cls['y'] && a.cls['y'] != 0,
              "what folds");
        CHECK(a.cls['`'] == 0 && a.cls['{'] == 0 && a.cls[0xE0] == 0, "the dead class");
        const Auto b({B("[^a]")}, BZR_FOLD_ASCII, 0);
        CHECK(b.ok && b.cls['a'] == 0 && b.cls['A'] == 0 && b.cls['\n'] != 0 && b.cls['b'] != 0, "a class is folded, then negated, and takes 0x0A");
        const Auto c({B(".")}, 0, 0), d({B(".")}, BZR_DOTALL, 0);
        CHECK(c.ok && c.cls['\n'] == 0 && c.plan.classes == 2 && d.ok && d.plan.classes == 1 && d.cls['\n'] == 0, "the dot; with every byte taken class 0 is an ordinary one");
    }
    // exactly 65,535 states beyond the root from exactly 65,536 NFA positions: 256 literal words that share nothing, the word of byte
    // i that byte 256 times, the first two an alternation in one expression, so that they end in one state.  Every expression has
    // its own terminal and nothing else merges.  The same words as 256 expressions: 65,536 states, refused.
    {
        Pats words;
        for (uint32_t i = 0; i < 256; i++) {
            std::string w;
            char q[8];
            snprintf(q, sizeof q, "\\x%02x", i);
            for (uint32_t j = 0; j < 256; j++) w += q;
            words.push_back(Bytes(w.begin(), w.end()));
        }
        Pats joined(words.begin() + 1, words.end());
        joined[0].insert(joined[0].begin(), '|');
        joined[0].insert(joined[0].begin(), words[0].begin(), words[0].end());
        const Auto a(joined, 0, 0);
        CHECK(a.ok, "65,535 states beyond the root are accepted: %s", a.why.c_str());
        table_invariants(a, "the largest automaton");
        CHECK(a.plan.in_lds == 0 && a.plan.states == 65536 && a.plan.classes == 256 && a.plan.unbounded == 0 && a.plan.max_len == 256, "the largest automaton: %u rows",
              a.plan.states);
        const Bytes t(256, 254);
        uint32_t pat = 0, len = 0;
        CHECK(a.walk(t.data(), 0, t.size(), &pat, &len) && len == 256 && pat == 253, "its last but one word is found");
        const Auto b(words, 0, 0);
        CHECK(!b.ok && b.why.find("65535 states") != std::string::npos, "one state more is refused: %s", b.why.c_str());
    }
    // the blow-up comes back at once
    {
        const clock_t t0 = clock();
        const Auto a({B("(a|b)*a(a|b){16}")}, 0, 0);
        CHECK(!a.ok && a.why.find("65535 states") != std::string::npos, "the blow-up is refused: %s", a.why.c_str());
        const Auto b({B("a|((a{256}){256}){256}")}, 0, 0);
        CHECK(!b.ok && b.why.find("positions") != std::string::npos, "the NFA bound: %s", b.why.c_str());
        const Auto c({B("(((((a?){256}){256}){256}){256}){256}b")}, 0, 0);
        CHECK(!c.ok && c.why.find("positions") != std::string::npos, "the NFA bound: %s", c.why.c_str());
        CHECK((double)(clock() - t0) / CLOCKS_PER_SEC < 20.0, "promptly");
    }
    printf("compile: held, %llu starts checked, %llu live, %llu seeded cases above a bound\n", (ull)checked, (ull)live, (ull)refused_big);
}

// ---- (b) the device: scan_host.h's model with BzrMatcher<true / false, false> ---------------------------------------------------------
static GrepTruth grep_naive(const Bytes &text, const Auto &s, uint32_t delim, uint32_t invert)
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
template <bool L>
static void grep_auto(const Bytes &text, const Auto &set, uint32_t delim, uint32_t invert, const std::vector<uint64_t> &blocks, int out_kind, int ent_kind)
{
    grep_call(text, grep_naive(text, set, delim, invert), [&](const BzgWindow &w) { return set.matcher<L>(delim, w.n); }, set.plan.max_len, invert,
              (uint8_t)(delim == 0xEE ? 0xED : 0xEE), blocks, out_kind, ent_kind);
}

// one raw search call with `max` hit slots; returns the hits
template <bool L>
static uint64_t search_raw(const Bytes &src, const Auto &set, uint32_t delim, bool records, uint64_t max)
{
    const uint64_t n = src.size();
    const Text text(src.data(), n);
    BzmSetWalk walk;
    walk.begin(set.plan.max_len, 0, max, 0, n, 0, 0);
    uint64_t lim = 0, hits, delims;
    const BzfWindow w = walk.window_set(n, true, &lim);
    CHECK(lim == n || w.s_hi == w.s_lo, "the raw window ends at the text's end");
    std::vector<BzmHit> out;
    search_run(text.p, w, set.matcher<L>(delim, lim), records, walk, out, &hits, &delims);
    same_hits(out, set.naive(text.p, n, 0, n, records, delim), hits, max, "raw", n);
    CHECK(!records || delims == (uint64_t)std::count(text.p, text.p + n, (uint8_t)delim), "raw (%llu): delimiters", (ull)n);
    return hits;
}
// both variants where the table fits the LDS, the HBM one alone where it does not (the library never stages a larger table)
static uint64_t search_both(const Bytes &src, const Auto &set, uint32_t delim, bool records, uint64_t max)
{
    const uint64_t h = search_raw<false>(src, set, delim, records, max);
    if (set.plan.table.size() <= BZR_LDS_ROWS) CHECK(search_raw<true>(src, set, delim, records, max) == h, "the two variants agree");
    return h;
}
static void grep_both(const Bytes &text, const Auto &set, uint32_t delim, uint32_t invert, const std::vector<uint64_t> &blocks, int out_kind, int ent_kind)
{
    grep_auto<false>(text, set, delim, invert, blocks, out_kind, ent_kind);
    if (set.plan.table.size() <= BZR_LDS_ROWS) grep_auto<true>(text, set, delim, invert, blocks, out_kind, ent_kind);
}

static void plant(Bytes &text, uint64_t at, const Bytes &p)
{
    if (at + p.size() <= text.size()) memcpy(&text[at], p.data(), p.size());
}
static Pats the_expressions(bool big)
{
    Pats e{B("[0-9]+"), B("err(or)?.*time"), B("(abc)+|a{2,3}"), B("\\s+"), B("r+"), B("ab"), B("a[a-c]")};
    if (big) { // a few hundred words: the table leaves the LDS bound
        std::string alt;
        for (int i = 0; i < 300; i++) {
            std::string w;
            for (int j = 0; j < 7; j++) w.push_back((char)('A' + below(26)));
            alt += (i ? "|" : "") + w;
        }
        e.push_back(Bytes(alt.begin(), alt.end()));
    }
    return e;
}

static void part_matcher()
{
    const uint64_t ns[] = {0, 1, 15, 16, 17, 4095, 4096, 4097, 8192, 12289};
    uint64_t cases = 0, found = 0, staged = 0;
    for (uint64_t n : ns)
        for (unsigned fold = 0; fold < 2; fold++)
            for (int big = 0; big < 2; big++) {
                const Auto set(the_expressions(big != 0), fold ? (unsigned)BZR_FOLD_ASCII : 0u, 0);
                CHECK(set.ok, "%s", set.why.c_str());
                CHECK((set.plan.table.size() <= BZR_LDS_ROWS) == !big && set.plan.in_lds == (uint32_t)!big, "the LDS bound: %zu entries", set.plan.table.size());
                staged += !big;
                Bytes text(n);
                for (auto &c : text) c = (uint8_t)"abcABC019 \nerotimERxyz"[below(22)];
                found += search_both(text, set, '\n', true, ~0ull), cases++;
                grep_both(text, set, '\n', 0, {}, 2, 2), grep_both(text, set, '\n', 1, {}, 2, 2);
                // the fixed places: a match of 256 bytes at offset 0, ending at byte n - 1, from 4095 to the halo's last byte, across a
                // thread edge and a wave edge; short ones at 15, 1023, 4095; the delimiter inside a match
                Bytes t2(n, '.');
                const Bytes run(256, fold ? 'R' : 'r');
                uint64_t last_end = 0, planted = 0;
                for (uint64_t e : {(uint64_t)0, (uint64_t)1024 - 100, (uint64_t)4095, (uint64_t)8192 - 255, n - 256})
                    if (e < n && e + 256 <= n && (!planted || e > last_end)) plant(t2, e, run), planted++, last_end = e + 256;
                for (uint64_t e : {(uint64_t)15, (uint64_t)1023, (uint64_t)4095 + 300})
                    if (e + 2 <= n && t2[e] == '.' && t2[e + 1] == '.') plant(t2, e, B("ab"));
                for (uint64_t at = 600; at + 3 <= n; at += 1000) plant(t2, at, B(" \n\t"));
                const uint64_t h = search_both(t2, set, '\n', true, ~0ull);
                CHECK(h >= planted, "planted %llu, found %llu", (ull)planted, (ull)h);
                found += h, cases++;
                grep_both(t2, set, '\n', 0, {}, 2, 2), grep_both(t2, set, '\n', 1, {}, 1, 0);
                // one byte value everywhere under x+: every start reports min(span, rest); every, three and no slots
                for (uint32_t span : {0u, 8u}) {
                    const Auto xs({B("x+")}, fold ? (unsigned)BZR_FOLD_ASCII : 0u, span);
                    const Bytes t3(n, fold ? 'X' : 'x');
                    CHECK(search_both(t3, xs, 'q', true, ~0ull) == n && search_both(t3, xs, 'x', true, 3) == n && search_both(t3, xs, 'x', false, 0) == n, "x+ over one byte value");
                    grep_both(t3, xs, fold ? 'X' : 'x', 0, {}, 2, 2), grep_both(t3, xs, 'q', 1, {}, 3, 3);
                    cases += 3;
                }
            }
    CHECK(staged > 0, "the LDS variant ran");
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
        const unsigned fold = (unsigned)below(2);
        const uint32_t span = below(3) ? 0 : 2 + (uint32_t)below(40);
        // a short match and a longer one at the same start: a run of a's, or "ab" and a tail that may hold the delimiter
        Pats exprs{below(2) ? B("a+") : B("ab(b|\\n)*"), B("b[ab]{0,9}x")};
        if (below(2)) exprs.push_back(B("[AB]{2,}"));
        const Auto set(exprs, fold ? (unsigned)BZR_FOLD_ASCII : 0u, span);
        CHECK(set.ok, "%s", set.why.c_str());
        const bool records = below(4) != 0;
        Bytes truth(total);
        for (auto &ch : truth) ch = (uint8_t)"abAx\n"[below(below(3) ? 5 : 4)];
        // on every block edge a long match that spans it; delimiters
        uint64_t edge = 0;
        std::vector<uint64_t> wins;
        for (size_t k = 0; k < nb; k++) {
            edge += blk[k];
            const uint64_t len = 2 + below(300), back = below(len + 1);
            if (below(4)) plant(truth, edge - std::min<uint64_t>(edge, back), Bytes(len, 'a'));
            if (edge < total && below(2)) truth[edge - below(2)] = '\n';
        }
        const size_t first = below(nb), last = first + 1 + below(nb - first);
        uint64_t start = 0, stop = 0;
        for (size_t k = 0; k < last; k++) (k < first ? start : stop) += blk[k];
        stop += start;
        const uint64_t lo = below(2) ? start : start + below(stop - start), hi = below(2) ? stop : lo + below(stop - lo + 1);
        const std::vector<BzmHit> want = set.naive(truth.data(), total, lo, hi, records, '\n');
        {   // a longer match cut by the range's end gives way to the longest that fits
            uint32_t p1, l1, p2, l2;
            for (uint64_t o = lo; o < hi && hi < total; o++)
                cut += set.walk(truth.data(), o, total, &p1, &l1) && set.walk(truth.data(), o, hi, &p2, &l2) && l2 < l1;
        }
        const uint64_t maxes[] = {~0ull, want.size(), want.size() ? want.size() - 1 : 0, 0, below(want.size() + 2)};
        const uint64_t max = maxes[below(5)];
        const uint64_t room = below(3) ? 1 + below(600) : 1 + below(20000);
        const size_t bmax = 1 + below(4);
        const bool lds = below(2) != 0;
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
            if (lds) search_run(d, w, set.matcher<true>('\n', lim), records, walk, out, &hits, &delims);
            else search_run(d, w, set.matcher<false>('\n', lim), records, walk, out, &hits, &delims);
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
        if (lds) grep_auto<true>(part, set, '\n', (uint32_t)below(2), wins, (int)below(5), (int)below(5));
        else grep_auto<false>(part, set, '\n', (uint32_t)below(2), wins, (int)below(5), (int)below(5));
    }
    CHECK(finished > cases / 4 && cut > 0, "the cases reach the edges: %llu finishing windows, %llu long matches cut by the range", (ull)finished, (ull)cut);
    printf("windows: %llu cases held, %llu windows, %llu finishing ones, %llu cut by the range\n", (ull)cases, (ull)windows, (ull)finished, (ull)cut);
}

// ---- hits EXPRFILE TEXTFILE FLAGS SPAN ----------------------------------------------------------------------------------------------
static Bytes slurp(const char *path)
{
    FILE *f = fopen(path, "rb");
    CHECK(f, "cannot open %s", path);
    Bytes b;
    uint8_t buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + k);
    fclose(f);
    return b;
}
static int mode_hits(char **argv)
{
    const Bytes ef = slurp(argv[2]), text = slurp(argv[3]);
    Pats exprs;
    for (size_t at = 0; at < ef.size();) {
        size_t end = at;
        while (end < ef.size() && ef[end] != '\n') end++;
        exprs.push_back(Bytes(ef.begin() + at, ef.begin() + end));
        at = end + 1;
    }
    const Auto a(exprs, (unsigned)strtoul(argv[4], nullptr, 10), (uint32_t)strtoul(argv[5], nullptr, 10));
    if (!a.ok) {
        fprintf(stderr, "%s\n", a.why.c_str());
        return 2;
    }
    const Text t(text.data(), text.size());
    BzmSetWalk walk;
    walk.begin(a.plan.max_len, 0, ~0ull, 0, text.size(), 0, 0);
    uint64_t lim = 0, hits, delims;
    const BzfWindow w = walk.window_set(text.size(), true, &lim);
    std::vector<BzmHit> out;
    if (a.plan.in_lds) search_run(t.p, w, a.matcher<true>('\n', lim), false, walk, out, &hits, &delims);
    else search_run(t.p, w, a.matcher<false>('\n', lim), false, walk, out, &hits, &delims);
    for (const BzmHit &h : out) printf("%llu %u %u\n", (ull)h.off, h.pattern, h.len);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 6 && !strcmp(argv[1], "hits")) return mode_hits(argv);
    rng_state = argc > 1 ? strtoull(argv[1], nullptr, 10) * 0x9E3779B97F4A7C15ull + 1 : 1;
    const uint64_t cases = argc > 2 ? strtoull(argv[2], nullptr, 10) : 200;
    part_compile(cases / 2);
    part_matcher();
    part_windows(cases);
    return 0;
}
