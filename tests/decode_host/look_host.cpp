// look_host.cpp -- anchors and word boundaries of the device regex without a device, built with g++ -fsanitize=address,undefined.
// (a) The compile of banzai_amd/csrc/regex_plan.h with assertions admitted, against a naive matcher over the harness's OWN expression
//     trees: seeded trees that hold ^ $ \A \Z \b \B in leading, inner and trailing places, matched here on the tree at every offset
//     of seeded texts with two bounds and two spans; the word and line wraps; the identity of the plan for lists without assertions;
//     the refusals without the syntax bit, the empty matches, a state count that crosses the bound only because of the contexts.
// (b) The look-around matcher of banzai_amd/csrc/regex_core.h -- BzrMatcher<true, true> and <false, true>, the kernels' own text -- thread by
//     thread and tile by tile over a model of the LDS: search and grep, the fixed places of the two extra bytes.
// (c) The windows: BzmSetWalk with both looks (search_plan.h) and BzgWalk (grep_plan.h) with (b) as the device, against brute force per output
//     byte, the decoded range widened as decode_range_sink_run widens it.
//
//   look_host <seed> <cases>                                exit status 0: everything held
//   look_host hits EXPRFILE TEXTFILE FLAGS SPAN SYNTAX      one expression a line; prints "off pattern len" for every hit of the text
#define HOST_NAME "look_host"
#include <time.h>

#include <bitset>
#include <set>
#include <string>

#include "../../include/bzhip.h"
#include "../../banzai_amd/csrc/regex_core.h"
#include "../../banzai_amd/csrc/regex_plan.h"
#include "regex_ex_host.h"
#include "scan_host.h"

typedef std::vector<Bytes> Pats;

static_assert(sizeof(bzh_regex_look) == 16 && sizeof(bzh_regex_info) == 40, "the two records");
static_assert((uint32_t)BZR_CTX_EDGE == (uint32_t)BZR_LOOK_EDGE && (uint32_t)BZR_CTX_NL == (uint32_t)BZR_LOOK_NL && (uint32_t)BZR_CTX_WORD == (uint32_t)BZR_LOOK_WORD &&
                  (uint32_t)BZR_CTX_OTHER == (uint32_t)BZR_LOOK_OTHER,
              "one numbering of the contexts");
static_assert(BZF_TILE - 1 + BZF_MAX_PATTERN == BZF_TILE + BZF_MAX_PATTERN - 1, "a match of 256 bytes from tile byte 4,095 looks ahead at the tile array's last byte");

static Bytes B(const char *s) { return Bytes(s, s + strlen(s)); }

// ---- the harness's own expressions ---------------------------------------------------------------------------------------------------
static const char ALPHA[] = "abAB01 _\n-z";
static Ex lit(uint8_t b)
{
    Ex e;
    e.set[b] = true;
    char q[8];
    if (strchr("\\.[]()|*+?{}^$-/", b)) snprintf(q, sizeof q, "\\%c", b), e.text = q;
    else if (b == '\n') e.text = "\\n";
    else e.text = std::string(1, (char)b);
    return e;
}
static Ex look_ex(char c)
{
    Ex e;
    e.kind = Ex::LOOK, e.look = c;
    e.text = c == '^' || c == '$' ? std::string(1, c) : std::string("\\") + c;
    return e;
}
static Ex random_look() { return look_ex("^$AZbB^$bB"[below(10)]); }
static Ex random_set(bool dotall)
{
    Ex e;
    const uint64_t k = below(8);
    if (k < 5) return lit((uint8_t)ALPHA[below(sizeof ALPHA - 1)]);
    if (k == 5) {
        for (uint32_t b = 0; b < 256; b++) e.set[b] = dotall || b != '\n';
        e.text = ".";
        return e;
    }
    if (k == 6) {
        for (uint32_t b = 0; b < 256; b++) e.set[b] = wordb((uint8_t)b);
        e.text = "\\w";
        return e;
    }
    e.neg = below(2) == 0;
    e.text = e.neg ? "[^a-b\\n]" : "[a-b\\n]";
    e.set['a'] = e.set['b'] = e.set['\n'] = true;
    return e;
}
static Ex random_ex(uint32_t depth, bool dotall)
{
    const uint64_t k = depth == 0 ? 0 : below(8);
    Ex e;
    if (k < 2) return random_set(dotall);
    if (k < 5) { // a sequence, assertions in leading, inner and trailing places
        e.kind = Ex::CAT;
        if (below(3) == 0) e.kids.push_back(random_look());
        for (uint64_t n = 2 + below(3); n > 0; n--) {
            e.kids.push_back(random_ex(depth - 1, dotall));
            if (n > 1 && below(4) == 0) e.kids.push_back(random_look());
        }
        if (below(3) == 0) e.kids.push_back(random_look());
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
static Ex wrapped(const Ex &e, unsigned syntax) // the word and the line wrap as trees
{
    if (!(syntax & (BZR_SYN_WORD | BZR_SYN_LINE))) return e;
    Ex c;
    c.kind = Ex::CAT;
    c.kids = {look_ex(syntax & BZR_SYN_WORD ? '<' : '^'), e, look_ex(syntax & BZR_SYN_WORD ? '>' : '$')};
    return c;
}

// ---- a compiled automaton as the device holds it --------------------------------------------------------------------------------------
struct Auto {
    BzrPlan plan;
    uint8_t *cls = nullptr, *acc_mask = nullptr;
    uint16_t *first = nullptr, *table = nullptr;
    uint32_t *pat_no = nullptr, *pat_ctx = nullptr;
    uint32_t ctx_row = 0;
    bool ok = false;
    std::string why;
    Auto(const Pats &exprs, unsigned flags, uint32_t span, unsigned syntax)
    {
        std::vector<const uint8_t *> ptr;
        std::vector<size_t> len;
        for (const Bytes &p : exprs) ptr.push_back(p.data()), len.push_back(p.size());
        char err[200] = "";
        ok = bzr_compile_ex(ptr.data(), len.data(), exprs.size(), flags, span, syntax, plan, err, sizeof err);
        why = err;
        if (!ok) return;
        cls = exact(plan.cls, 256), first = exact(plan.first, 256 * (size_t)plan.contexts);
        table = exact(plan.table.data(), plan.table.size()), pat_no = exact(plan.pat_no.data(), plan.pat_no.size());
        acc_mask = exact(plan.acc_mask.data(), plan.acc_mask.size()), pat_ctx = exact(plan.pat_ctx.data(), plan.pat_ctx.size());
        for (uint32_t c = 0; c < 4; c++) ctx_row |= (uint32_t)plan.ctx_row[c] << (8 * c);
    }
    ~Auto() { free(cls), free(first), free(table), free(pat_no), free(acc_mask), free(pat_ctx); }
    Auto(const Auto &) = delete;
    bool looks() const { return plan.look_behind || plan.look_ahead; }
    template <bool L>
    BzrMatcher<L, true> matcher(uint32_t delim, uint64_t lim, uint64_t n, uint64_t edge_lo, uint32_t ctx_lo) const
    {
        return BzrMatcher<L, true>{{BzrAuto{BzmSet{cls, first, table, pat_no, plan.classes, plan.nterm, plan.max_len, delim, lim}, plan.states * plan.classes},
                                        BzrLook{acc_mask, pat_ctx, plan.contexts, ctx_row, plan.look_ahead, ctx_lo, edge_lo, n}}, {}};
    }
    // the table walked without a tile, every invariant checked on the way: the hit at text[o ..) of text[0, n), bounded by lim
    bool walk(const uint8_t *text, uint64_t n, uint64_t o, uint64_t lim, uint32_t *pattern, uint32_t *len) const
    {
        CHECK(looks() && plan.acc_mask.size() == plan.nterm && plan.pat_ctx.size() == 4u * plan.nterm, "the look-around records");
        const uint32_t pc = o == 0 ? (uint32_t)BZR_CTX_EDGE : bzr_ctx_of(text[o - 1]);
        CHECK(plan.ctx_row[pc] < plan.contexts && plan.contexts <= 4, "a start row");
        uint32_t st = 0;
        bool hit = false;
        for (uint32_t depth = 0; o + depth < lim && depth < plan.max_len; depth++) {
            const uint32_t c = cls[text[o + depth]];
            const size_t at = (size_t)st * plan.classes + c;
            CHECK(at < plan.table.size(), "the walk leaves the table");
            st = depth ? table[at] : first[256 * plan.ctx_row[pc] + text[o + depth]];
            if (!st) break;
            CHECK(st < plan.states, "state %u of %u", st, plan.states);
            if (st <= plan.nterm) {
                const uint32_t nc = o + depth + 1 == n ? (uint32_t)BZR_CTX_EDGE : bzr_ctx_of(text[o + depth + 1]);
                if (acc_mask[st - 1] >> nc & 1u) hit = true, *pattern = pat_ctx[4 * (st - 1) + nc], *len = depth + 1;
            }
        }
        return hit;
    }
    std::vector<BzmHit> naive(const uint8_t *text, uint64_t n, uint64_t lo, uint64_t hi, bool records, uint32_t delim) const
    {
        std::vector<BzmHit> v;
        hi = std::min(hi, n);
        uint64_t rec = 0;
        for (uint64_t o = 0; o < hi; o++) {
            uint32_t pat, len;
            if (o >= lo && walk(text, n, o, hi, &pat, &len)) v.push_back(BzmHit{o, records ? rec : 0, pat, len});
            rec += text[o] == delim;
        }
        return v;
    }
    bool any_at(const uint8_t *text, uint64_t n, uint64_t o) const
    {
        uint32_t pat, len;
        return walk(text, n, o, n, &pat, &len);
    }
};

// ---- (a) the compile -----------------------------------------------------------------------------------------------------------------
static void refused(const char *expr, unsigned syntax, const char *needle)
{
    const Auto a({B(expr)}, 0, 0, syntax);
    CHECK(!a.ok && a.why.find(needle) != std::string::npos, "\"%s\" under syntax %u refused with \"%s\", want \"%s\"", expr, syntax, a.why.c_str(), needle);
}
static void same_plan(const Pats &exprs, unsigned flags, uint32_t span)
{
    const Auto a(exprs, flags, span, 0), b(exprs, flags, span, BZR_SYN_ASSERT);
    CHECK(a.ok == b.ok && a.why == b.why, "a list without assertions: the same verdict");
    if (!a.ok) return;
    const BzrPlan &p = a.plan, &q = b.plan;
    CHECK(p.expressions == q.expressions && p.min_len == q.min_len && p.max_len == q.max_len && p.max_span == q.max_span && p.states == q.states && p.classes == q.classes &&
              p.nterm == q.nterm && p.unbounded == q.unbounded && p.in_lds == q.in_lds,
          "a list without assertions: the same figures");
    CHECK(!memcmp(p.cls, q.cls, sizeof p.cls) && !memcmp(p.first, q.first, sizeof p.first) && p.table == q.table && p.pat_no == q.pat_no, "... the same cls, first, table, pat_no");
    CHECK(q.look_behind == 0 && q.look_ahead == 0 && q.contexts == 1 && q.acc_mask.empty() && q.pat_ctx.empty(), "... and it looks at nothing");
}
static void part_compile(uint64_t cases)
{
    for (uint32_t b = 0; b < 256; b++) CHECK(bzr_ctx(b) == bzr_ctx_of(b), "the device and the compile name the context of byte %u alike", b);
    uint64_t checked = 0, live = 0, refused_big = 0, with_look = 0, depends = 0, contradictory = 0;
    for (uint64_t c = 0; c < cases; c++) {
        const unsigned flags = (unsigned)below(4);
        const bool fold = flags & BZR_FOLD_ASCII, dotall = (flags & BZR_DOTALL) != 0;
        const unsigned syntax = BZR_SYN_ASSERT | (below(5) == 0 ? (below(2) ? (unsigned)BZR_SYN_WORD : (unsigned)BZR_SYN_LINE) : 0u);
        std::vector<Ex> exs;
        Pats exprs;
        bool any_look = (syntax & ~(unsigned)BZR_SYN_ASSERT) != 0;
        for (uint64_t k = 1 + below(3); k > 0; k--) {
            Ex e = random_ex(1 + (uint32_t)below(3), dotall);
            while (min_len(e) == 0 || min_len(e) > 5) e = random_ex(1 + (uint32_t)below(3), dotall);
            const std::string s = print(e, true);
            any_look = any_look || has_look(e);
            exs.push_back(wrapped(e, syntax)), exprs.push_back(Bytes(s.begin(), s.end()));
        }
        if (!any_look) {
            same_plan(exprs, flags, 256), same_plan(exprs, flags, 5);
            continue;
        }
        with_look++;
        Bytes text(100 + below(100));
        for (auto &ch : text) ch = below(12) ? (uint8_t)ALPHA[below(sizeof ALPHA - 1)] : (uint8_t)below(256);
        const Text t(text.data(), text.size());
        const uint64_t n = text.size();
        for (uint32_t span : {256u, 5u}) {
            const Auto a(exprs, flags, span, syntax);
            if (!a.ok) {
                if (a.why.find("contradict") != std::string::npos) { // (a^b: the tree agrees that nothing matches)
                    for (uint64_t o = 0; o < n; o++)
                        for (const Ex &e : exs) CHECK(ends(e, t.p, n, n, Ends{o}, fold).empty(), "case %llu: refused as contradictory, and matches at %llu", (ull)c, (ull)o);
                    contradictory++;
                    continue;
                }
                CHECK(a.why.find("states") != std::string::npos || a.why.find("positions") != std::string::npos, "case %llu: %s", (ull)c, a.why.c_str());
                refused_big++;
                continue;
            }
            CHECK(a.looks() && a.plan.nterm >= 1 && a.plan.nterm < a.plan.states, "case %llu (%s): an automaton with assertions looks somewhere: %u %u, %u terminals of %u rows", (ull)c,
                  (const char *)std::string(exprs[0].begin(), exprs[0].end()).c_str(), a.plan.look_behind, a.plan.look_ahead, a.plan.nterm, a.plan.states);
            bool longer = false;
            for (uint64_t lim : {n, n / 2})
                for (uint64_t o = 0; o < lim; o++) {
                    uint64_t best = 0;
                    uint32_t who = 0;
                    for (uint32_t j = 0; j < exs.size(); j++) {
                        const Ends en = ends(exs[j], t.p, n, lim, Ends{o}, fold);
                        for (uint64_t e : en) {
                            if (e - o > span) longer = true;
                            else if (e > o && e - o > best) best = e - o, who = j;
                        }
                    }
                    uint32_t pat = 0, len = 0;
                    const bool hit = a.walk(t.p, n, o, lim, &pat, &len);
                    CHECK(hit == (best > 0) && (!hit || (len == best && pat == who)), "case %llu (%s ...) flags %u span %u syntax %u at %llu: the table says %d (%u, %u), the tree (%u, %llu)",
                          (ull)c, (const char *)std::string(exprs[0].begin(), exprs[0].end()).c_str(), flags, span, syntax, (ull)o, (int)hit, pat, len, who, (ull)best);
                    checked++, live += hit;
                }
            CHECK(!longer || a.plan.unbounded, "case %llu: a match above the span, and unbounded is 0", (ull)c);
            depends += a.plan.contexts > 1;
        }
    }
    CHECK(with_look > cases / 4 && live > checked / 200 && depends > 0, "the seeded cases hold assertions and match somewhere: %llu lists, %llu of %llu starts, %llu with several start rows",
          (ull)with_look, (ull)live, (ull)checked, (ull)depends);

    // the figures: an assertion consumes nothing
    {
        const Auto a({B("^ab$")}, 0, 0, BZR_SYN_ASSERT), b({B("\\bfoo\\b")}, 0, 0, BZR_SYN_ASSERT), c({B("a+$")}, 0, 0, BZR_SYN_ASSERT), d({B("\\Aa")}, 0, 0, BZR_SYN_ASSERT);
        CHECK(a.ok && a.plan.min_len == 2 && a.plan.max_len == 2 && a.plan.look_behind == 1 && a.plan.look_ahead == 1 && a.plan.contexts == 2, "^ab$: %s", a.why.c_str());
        CHECK(b.ok && b.plan.min_len == 3 && b.plan.max_len == 3 && b.plan.look_behind == 1 && b.plan.look_ahead == 1 && b.plan.contexts == 2, "\\bfoo\\b");
        CHECK(c.ok && c.plan.look_behind == 0 && c.plan.look_ahead == 1 && c.plan.contexts == 1 && c.plan.unbounded == 1, "a+$ looks ahead only");
        CHECK(d.ok && d.plan.look_behind == 1 && d.plan.look_ahead == 0 && d.plan.contexts == 2, "\\Aa looks behind only");
        const Auto w({B("ab")}, 0, 0, BZR_SYN_WORD), x({B("ab")}, 0, 0, BZR_SYN_LINE);
        CHECK(w.ok && w.looks() && w.plan.max_len == 2 && x.ok && x.looks() && x.plan.contexts == 2, "the wraps work without the assertion bit");
    }
    // the identity for fixed lists
    same_plan({B("[0-9]+"), B("err(or)?.*time"), B("(abc)+|a{2,3}"), B("\\s+")}, 0, 0);
    same_plan({B("(ab)*c")}, BZR_FOLD_ASCII, 16);
    same_plan({B("\\^a\\$"), B("[$^]b")}, 0, 0);
    // the refusals without the syntax bit, byte for byte
    refused("^a", 0, "expression 0, byte 0: anchors are not supported");
    refused("a$", 0, "expression 0, byte 1: anchors are not supported");
    refused("a\\b", 0, "expression 0, byte 1: anchors and \\b are not supported");
    refused("\\Aa", 0, "expression 0, byte 0: anchors and \\b are not supported");
    refused("a\\Z", 0, "expression 0, byte 1: anchors and \\b are not supported");
    refused("a\\B", 0, "expression 0, byte 1: anchors and \\b are not supported");
    refused("^a", BZR_SYN_WORD, "anchors are not supported");
    // what stays refused with it
    refused("[\\b]a", BZR_SYN_ASSERT, "anchors and \\b are not supported");
    refused("a^*", BZR_SYN_ASSERT, "nothing to repeat");
    refused("\\b+a", BZR_SYN_ASSERT, "nothing to repeat");
    refused("^", BZR_SYN_ASSERT, "it matches the empty string");
    refused("^$", BZR_SYN_ASSERT, "it matches the empty string");
    refused("\\b", BZR_SYN_ASSERT, "it matches the empty string");
    refused("^a*$", BZR_SYN_ASSERT, "it matches the empty string");
    refused("a*", BZR_SYN_LINE, "it matches the empty string");
    refused("a^b", BZR_SYN_ASSERT, "contradict");
    refused("a", 8, "syntax");
    refused("a", BZR_SYN_WORD | BZR_SYN_LINE, "exclude each other");
    // a state count that crosses the bound only because of the contexts: (a|b)*a(a|b){14} has 2^15 + ... states and is accepted; with
    // a \B between the repeats the state names the context of its last byte as well
    {
        const clock_t t0 = clock();
        const Auto a({B("[xa\\n-]*x[xa\\n-]{14}")}, 0, 0, BZR_SYN_ASSERT), b({B("([xa\\n-]|\\bq)*x[xa\\n-]{14}")}, 0, 0, BZR_SYN_ASSERT);
        CHECK(a.ok && !a.looks(), "without an assertion the automaton fits: %s", a.why.c_str());
        CHECK(!b.ok && b.why.find("65535 states") != std::string::npos, "with the contexts it does not: %s", b.why.c_str());
        CHECK((double)(clock() - t0) / CLOCKS_PER_SEC < 60.0, "promptly");
    }
    printf("compile: held, %llu starts checked, %llu live, %llu lists with assertions, %llu above a bound, %llu contradictory\n", (ull)checked, (ull)live, (ull)with_look,
           (ull)refused_big, (ull)contradictory);
}

// ---- (b) the device: scan_host.h's model with BzrMatcher<true / false, true>.  What no thread stores is 'w' here (main): a word byte,
// so a look-ahead that reads it, or the zero behind the text, shows ----------------------------------------------------------------------
static GrepTruth grep_naive(const Bytes &text, const Auto &s, uint32_t delim, uint32_t invert)
{
    GrepTruth tr;
    const uint64_t n = text.size();
    uint64_t start = 0, rec = 0;
    auto close = [&](uint64_t end) {
        bool hit = false;
        for (uint64_t o = start; o < end && !hit; o++) hit = s.any_at(text.data(), n, o);
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
// one grep call over the whole of `text`; blocks: the windows' new bytes (empty: the raw call)
template <bool L>
static void grep_auto(const Bytes &text, const Auto &set, uint32_t delim, uint32_t invert, const std::vector<uint64_t> &blocks)
{
    // grep.hip's pick: the text begins at a record start; GrepSink: the hold-back grows by the byte behind a match
    grep_call(text, grep_naive(text, set, delim, invert),
              [&](const BzgWindow &w) { return set.matcher<L>(delim, w.n, w.n, w.t_lo, w.off_base + w.t_lo == 0 ? (uint32_t)BZR_LOOK_EDGE : bzr_ctx(delim)); },
              set.plan.max_len + set.plan.look_ahead, invert, 'w', blocks, 2, 2);
}

// one raw search call with `max` hit slots; returns the hits
template <bool L>
static uint64_t search_raw(const Bytes &src, const Auto &set, uint32_t delim, bool records, uint64_t max)
{
    const uint64_t n = src.size();
    const Text text(src.data(), n, 'w');
    BzmSetWalk walk;
    walk.begin(set.plan.max_len, 0, max, 0, n, 0, 0);
    walk.begin_look(set.plan.look_behind, set.plan.look_ahead);
    uint64_t lim = 0, hits, delims;
    const BzfWindow w = walk.window_set(n, true, &lim);
    std::vector<BzmHit> out;
    search_run(text.p, w, set.matcher<L>(delim, lim, w.n, 0 - w.off_base, BZR_LOOK_EDGE), records, walk, out, &hits, &delims);
    same_hits(out, set.naive(text.p, n, 0, n, records, delim), hits, max, "raw", n);
    return hits;
}
static uint64_t search_both(const Bytes &src, const Auto &set, uint32_t delim, bool records, uint64_t max)
{
    const uint64_t h = search_raw<false>(src, set, delim, records, max);
    if (set.plan.table.size() <= BZR_LDS_ROWS) CHECK(search_raw<true>(src, set, delim, records, max) == h, "the two variants agree");
    return h;
}
static void grep_both(const Bytes &text, const Auto &set, uint32_t delim, uint32_t invert, const std::vector<uint64_t> &blocks)
{
    grep_auto<false>(text, set, delim, invert, blocks);
    if (set.plan.table.size() <= BZR_LDS_ROWS) grep_auto<true>(text, set, delim, invert, blocks);
}
static void plant(Bytes &text, uint64_t at, const Bytes &p)
{
    if (at + p.size() <= text.size()) memcpy(&text[at], p.data(), p.size());
}
static Pats the_expressions(bool big)
{
    Pats e{B("^[a-z]+"), B("[0-9]+$"), B("\\berr(or)?\\b"), B("a\\B."), B("\\A.+"), B("x+\\Z"), B("(^|\\t)time"), B("a$\\n^b"), B("r+$")};
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
static uint64_t hits_at(const Bytes &text, const Auto &set, uint64_t at, uint32_t len)
{
    uint32_t p, l;
    return at < text.size() && set.walk(text.data(), text.size(), at, text.size(), &p, &l) && l == len;
}

static void part_matcher()
{
    const uint64_t ns[] = {0, 1, 15, 16, 17, 4095, 4096, 4097, 8192, 12289};
    uint64_t cases = 0, found = 0;
    for (uint64_t n : ns)
        for (int big = 0; big < 2; big++) {
            const Auto set(the_expressions(big != 0), 0, 0, BZR_SYN_ASSERT);
            CHECK(set.ok && set.plan.look_behind && set.plan.look_ahead, "%s", set.why.c_str());
            CHECK((set.plan.table.size() <= BZR_LDS_ROWS) == !big && set.plan.in_lds == (uint32_t)!big, "the LDS bound: %zu entries", set.plan.table.size());
            Bytes text(n);
            for (auto &c : text) c = (uint8_t)"abcA 019 \n\terotimERxyz"[below(22)];
            found += search_both(text, set, '\n', true, ~0ull), cases++;
            grep_both(text, set, '\n', 0, {}), grep_both(text, set, '\n', 1, {}), grep_both(text, set, 'a', 0, {});
            // the fixed places.  ^: at offset 0, at 16 and 1024 (the byte in front lies in another thread, another wave), at 4096 and
            // 8192 (in the tile before).  $: a run that ends at byte n, one in front of a final 0x0A, one that ends at tile byte 4095
            // (the byte behind is the halo's first), and 256 bytes from 4095: the byte behind is the tile array's last
            {
                const Auto up({B("^ab"), B("x+$")}, 0, 0, BZR_SYN_ASSERT);
                Bytes t2(n, '.');
                uint64_t want = 0;
                for (uint64_t at : {(uint64_t)0, (uint64_t)16, (uint64_t)1024, (uint64_t)4096, (uint64_t)8192})
                    if (at + 2 <= n) {
                        plant(t2, at, B("ab"));
                        if (at) t2[at - 1] = '\n';
                        want++;
                    }
                if (n >= 4096 + 300) plant(t2, 4090, B("xx\n"));
                if (n > 20) plant(t2, n - 3, B("xxx"));
                const uint64_t h = search_both(t2, up, '\n', true, ~0ull);
                for (uint64_t at : {(uint64_t)0, (uint64_t)16, (uint64_t)1024, (uint64_t)4096, (uint64_t)8192})
                    if (at + 2 <= n) CHECK(hits_at(t2, up, at, 2), "^ab at %llu of %llu", (ull)at, (ull)n);
                if (n >= 4096 + 300) {
                    CHECK(hits_at(t2, up, 4090, 2), "x+$ in front of tile byte 4093");
                    Bytes t5(n, '.'); // (a text of its own: the run covers 4096)
                    plant(t5, 4095, Bytes(256, 'x')), t5[4095 + 256] = '\n';
                    search_both(t5, up, '\n', true, ~0ull);
                    CHECK(hits_at(t5, up, 4095, 256), "x+$ of 256 bytes from 4095: the byte behind is the tile array's last");
                    Bytes t6(n, '.');
                    plant(t6, 4000, Bytes(96, 'x')), t6[4096] = '\n';
                    search_both(t6, up, '\n', true, ~0ull), grep_both(t6, up, '\n', 0, {});
                    CHECK(hits_at(t6, up, 4095, 1) && hits_at(t6, up, 4000, 96), "x+$ that ends at tile byte 4095: the byte behind is the halo's first");
                    search_both(t5, up, '\n', true, ~0ull), grep_both(t5, up, '\n', 0, {});
                }
                if (n > 20) CHECK(hits_at(t2, up, n - 3, 3), "x+$ at the text's end");
                CHECK(h >= want, "planted %llu, found %llu", (ull)want, (ull)h);
                found += h, cases++;
                grep_both(t2, up, '\n', 0, {}), grep_both(t2, up, '\n', 1, {});
                if (n > 20) { // ... and in front of a final 0x0A
                    t2[n - 1] = '\n';
                    search_both(t2, up, '\n', false, ~0ull);
                    CHECK(hits_at(t2, up, n - 3, 2), "x+$ in front of the final 0x0A");
                }
            }
            // the zero behind the text and the bytes no thread stored are no neighbours: a text that ends in a word byte under \b
            // and \Z, a text of one byte value under $
            {
                const Auto wb({B("w+\\b"), B("q\\Z")}, 0, 0, BZR_SYN_ASSERT), ds({B("w$")}, 0, 0, BZR_SYN_ASSERT);
                Bytes t3(n, 'w');
                if (n) t3[n - 1] = below(2) ? 'q' : 'w';
                CHECK(search_both(t3, wb, '\n', false, ~0ull) == (n && t3[n - 1] == 'q' ? 1 : std::min<uint64_t>(n, 256)), "w+\\b and q\\Z over a run of w, n = %llu", (ull)n);
                const Bytes t4(n, 'w');
                CHECK(search_both(t4, ds, '\n', false, 3) == (n ? 1u : 0u), "w$ over a run of w, n = %llu", (ull)n);
                cases += 2;
            }
        }
    // the wraps
    {
        const Auto w({B("er+"), B("[0-9]")}, 0, 0, BZR_SYN_WORD), x({B("[a-z ]+"), B("x")}, 0, 0, BZR_SYN_LINE);
        Bytes text(9000);
        for (auto &c : text) c = (uint8_t)"er 1\nx.r"[below(8)];
        found += search_both(text, w, '\n', true, ~0ull) + search_both(text, x, '\n', true, ~0ull), cases += 2;
        grep_both(text, w, '\n', 0, {}), grep_both(text, x, '\n', 1, {});
    }
    printf("matcher: %llu search cases held, %llu hits\n", (ull)cases, (ull)found);
}

// ---- (c) windows -----------------------------------------------------------------------------------------------------------------------
static void part_windows(uint64_t cases)
{
    uint64_t windows = 0, finished = 0, tight = 0, found = 0;
    for (uint64_t c = 0; c < cases; c++) {
        const size_t nb = 1 + below(7);
        std::vector<uint64_t> blk(nb), edge_of(nb + 1, 0);
        uint64_t total = 0;
        for (size_t k = 0; k < nb; k++) blk[k] = below(3) ? 1 + below(300) : 1 + below(9000), total += blk[k], edge_of[k + 1] = total;
        const uint32_t span = below(3) ? 0 : 3 + (uint32_t)below(40); // (a$\n^b takes three bytes)
        static const char *const lists[][3] = {{"^a+", "b+$", "\\bab\\b"}, {"^[ab]+$", "x\\B.", "\\Aa"}, {"a$\\n^b", "(^|x)b+", "[ab]+\\Z"}, {"a+", "b\\b", nullptr}, {"^a", nullptr, nullptr}};
        const uint64_t li = below(5);
        Pats exprs;
        for (const char *e : lists[li])
            if (e) exprs.push_back(B(e));
        const unsigned syntax = BZR_SYN_ASSERT | (below(6) == 0 ? (below(2) ? (unsigned)BZR_SYN_WORD : (unsigned)BZR_SYN_LINE) : 0u);
        const Auto set(exprs, 0, span, syntax);
        CHECK(set.ok && set.looks(), "%s", set.why.c_str());
        const bool records = below(4) != 0;
        Bytes truth(total);
        for (auto &ch : truth) ch = (uint8_t)"abAx\n "[below(below(3) ? 6 : 4)];
        // on every block edge a line end, a line start or a long run that spans it
        for (size_t k = 1; k <= nb; k++) {
            const uint64_t edge = edge_of[k], what = below(5);
            if (what == 0 && edge < total) truth[edge] = '\n';
            else if (what == 1) truth[edge - 1] = '\n';
            else if (what == 2) {
                const uint64_t len = 2 + below(300), back = below(len + 1);
                plant(truth, edge - std::min<uint64_t>(edge, back), Bytes(len, 'a'));
            }
        }
        // the wanted range, and the blocks of the decoded one: widened by what the automaton looks at, clipped to the output
        uint64_t lo, hi;
        if (below(3) == 0) { // its first byte a block's first, its last a block's last
            const size_t f = below(nb), l = f + 1 + below(nb - f);
            lo = edge_of[f], hi = edge_of[l], tight++;
        } else {
            lo = below(total), hi = lo + 1 + below(total - lo);
        }
        const uint64_t w_lo = lo - std::min<uint64_t>(lo, set.plan.look_behind), w_hi = std::min(total, hi + set.plan.look_ahead);
        size_t first = 0, last = nb;
        while (edge_of[first + 1] <= w_lo) first++;
        while (edge_of[last - 1] >= w_hi) last--;
        const uint64_t start = edge_of[first], stop = edge_of[last];
        const std::vector<BzmHit> want = set.naive(truth.data(), total, lo, hi, records, '\n');
        found += want.size();
        const uint64_t maxes[] = {~0ull, want.size(), want.size() ? want.size() - 1 : 0, 0, below(want.size() + 2)};
        const uint64_t max = maxes[below(5)];
        const uint64_t room = below(3) ? 1 + below(600) : 1 + below(20000);
        const size_t bmax = 1 + below(4);
        const bool lds = below(2) != 0 && set.plan.table.size() <= BZR_LDS_ROWS;
        uint64_t rec_start = 0;
        for (uint64_t i = 0; i < start; i++) rec_start += truth[i] == '\n';
        BzmSetWalk walk;
        walk.begin(set.plan.max_len, BZF_FRONT, max, lo, hi, start, records ? rec_start : 0);
        walk.begin_look(set.plan.look_behind, set.plan.look_ahead);
        std::vector<BzmHit> got((size_t)std::min<uint64_t>(max, want.size() + 8), BzmHit{~0ull, ~0ull, ~0u, ~0u});
        Bytes carry;
        uint64_t at_out = start;
        std::vector<uint64_t> wins;
        auto run = [&](const uint8_t *d, const BzfWindow &w, uint64_t lim, uint64_t bytes, bool is_last) {
            CHECK(w.s_lo <= w.s_hi && w.s_hi <= lim && lim <= w.n, "window: starts [%llu, %llu) lim %llu n %llu", (ull)w.s_lo, (ull)w.s_hi, (ull)lim, (ull)w.n);
            CHECK(w.s_lo == w.s_hi || w.s_lo >= w.n - bytes - walk.carry + walk.ctxb, "a byte of context is no start");
            std::vector<BzmHit> out;
            uint64_t hits, delims;
            if (lds) search_run(d, w, set.matcher<true>('\n', lim, w.n, 0 - w.off_base, BZR_LOOK_EDGE), records, walk, out, &hits, &delims);
            else search_run(d, w, set.matcher<false>('\n', lim, w.n, 0 - w.off_base, BZR_LOOK_EDGE), records, walk, out, &hits, &delims);
            for (size_t i = 0; i < out.size(); i++) got.at((size_t)walk.rank + i) = out[i];
            walk.advance_set(bytes, hits, delims, is_last);
            windows++;
        };
        for (size_t at = first; at < last;) {
            uint64_t bytes = 0;
            size_t nbw = 0;
            while (at + nbw < last && nbw < bmax && (nbw == 0 || bytes + blk[at + nbw] <= room)) bytes += blk[at + nbw], nbw++;
            wins.push_back(bytes);
            const Text staging(BZF_FRONT + bytes, 'w');
            memset(staging.p, 'w', BZF_FRONT);
            CHECK(carry.size() == walk.carry && walk.carry <= 257 && walk.carry < BZF_FRONT, "the carry");
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
            const Text held(carry.data(), carry.size(), 'w');
            walk.front = walk.carry;
            uint64_t lim = 0;
            const BzfWindow w = walk.window_set(0, true, &lim);
            run(held.p, w, lim, 0, true);
            finished++;
        }
        same_hits(got, want, walk.rank, max, "windows", c);
        // the grep over the same windows (it takes the whole text of the blocks it is given: both edges are the text's)
        const Bytes part(truth.begin() + start, truth.begin() + stop);
        const uint32_t delim = below(4) ? '\n' : 'x';
        if (lds) grep_auto<true>(part, set, delim, (uint32_t)below(2), wins);
        else grep_auto<false>(part, set, delim, (uint32_t)below(2), wins);
    }
    CHECK(finished > cases / 4 && tight > cases / 6 && found > cases, "the cases reach the edges: %llu finishing windows, %llu ranges on block edges, %llu hits", (ull)finished,
          (ull)tight, (ull)found);
    printf("windows: %llu cases held, %llu windows, %llu finishing ones, %llu ranges on block edges, %llu hits\n", (ull)cases, (ull)windows, (ull)finished, (ull)tight, (ull)found);
}

// ---- hits EXPRFILE TEXTFILE FLAGS SPAN SYNTAX ---------------------------------------------------------------------------------------
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
    const Auto a(exprs, (unsigned)strtoul(argv[4], nullptr, 10), (uint32_t)strtoul(argv[5], nullptr, 10), (unsigned)strtoul(argv[6], nullptr, 10));
    if (!a.ok) {
        fprintf(stderr, "%s\n", a.why.c_str());
        return 2;
    }
    CHECK(a.looks(), "the hits mode is for automata that look around");
    const Text t(text.data(), text.size(), 'w');
    BzmSetWalk walk;
    walk.begin(a.plan.max_len, 0, ~0ull, 0, text.size(), 0, 0);
    walk.begin_look(a.plan.look_behind, a.plan.look_ahead);
    uint64_t lim = 0, hits, delims;
    const BzfWindow w = walk.window_set(text.size(), true, &lim);
    std::vector<BzmHit> out;
    if (a.plan.in_lds) search_run(t.p, w, a.matcher<true>('\n', lim, w.n, 0, BZR_LOOK_EDGE), false, walk, out, &hits, &delims);
    else search_run(t.p, w, a.matcher<false>('\n', lim, w.n, 0, BZR_LOOK_EDGE), false, walk, out, &hits, &delims);
    for (const BzmHit &h : out) printf("%llu %u %u\n", (ull)h.off, h.pattern, h.len);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 7 && !strcmp(argv[1], "hits")) return mode_hits(argv);
    poison_tile = poison_front = 'w';
    rng_state = argc > 1 ? strtoull(argv[1], nullptr, 10) * 0x9E3779B97F4A7C15ull + 1 : 1;
    const uint64_t cases = argc > 2 ? strtoull(argv[2], nullptr, 10) : 200;
    part_compile(cases);
    part_matcher();
    part_windows(cases);
    return 0;
}
