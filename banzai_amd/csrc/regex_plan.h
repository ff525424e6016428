// regex_plan.h -- 1 .. 65,536 regular expressions compiled into ONE automaton for their union, in the shape of patset_plan.h's trie:
// a class map, a first-step row and a dense 16-bit table, walked from every start position by the matcher of regex_core.h
// (bzh_regex_create, regex.hip).  Pure host C++17, no HIP in it: the library compiles it, and tests/decode_host/regex_host.cpp runs
// it under ASan and UBSan against a naive backtracking matcher.
//
// THE ROUTE: parse -> Thompson NFA (bounded repeats expanded) -> byte classes -> subset construction -> minimisation -> numbering.
//
// THE SYNTAX is a subset of Python's `re` on bytes: literal bytes; the escapes \\ \. \[ \] \( \) \| \* \+ \? \{ \} \^ \$ \- \/ \n \t
// \r \f \v \0 \xHH, and a backslash in front of any other ASCII byte that is no letter or digit (what re.escape writes); \d \D \w \W \s \S (ASCII, \s = [ \t\n\r\f\v]); `.` (any byte but 0x0A, any byte with BZR_DOTALL); [...] and
// [^...] with ranges and those escapes (a negated class does take 0x0A); ( ) and (?: ), both plain grouping; | ; ? * + {m} {m,}
// {m,n}.  With BZR_SYN_ASSERT the assertions ^ $ \A \Z \b \B, anywhere but in a class or under a quantifier (below: THE ASSERTIONS).
// Refused, naming the expression and the byte: without that bit anchors and \b, every other escape, backreferences, lookaround, lazy and
// possessive quantifiers, named groups, inline flags, a `{` that opens no well-formed bound, a bound above 256, an unbalanced
// bracket, an expression that matches the empty string, one whose shortest match exceeds max_span.  With BZR_FOLD_ASCII the bytes
// 'A'..'Z' and 'a'..'z' compare equal, in literals and in classes (a class is folded, then negated): re.IGNORECASE on bytes.
//
// THE BOUNDS: the NFA holds at most 65,536 positions (byte-consuming states) behind the expansion, the subset construction makes at
// most 65,535 states beyond the root; both stop and refuse the moment the bound is passed.
//
// THE TABLE keeps patset_plan.h's invariants, restated for cycles.  Row 0 is the root and no transition leads to it (the start
// subset, where it recurs as a target, gets a row of its own), so an entry 0 means "dead".  Terminal states are 1 .. nterm, and
// pat_no[st - 1] is the lowest-numbered expression that accepts in st (the minimisation's first partition separates states by
// it); the other rows follow, all in breadth-first order from the root.  Bytes no expression can take share the dead class 0.
// min_len: the shortest path to a terminal; max_len: min(the longest match, max_span); unbounded: some match could be longer than
// max_span -- a cycle on a path to a terminal, or an acyclic longest path above the span.
//
// THE ASSERTIONS (bzr_compile_ex with BZR_SYN_ASSERT; the word and the line wrap BZR_SYN_WORD / BZR_SYN_LINE put one in front of and
// one behind every expression).  An assertion sees the byte in front of its place and the byte behind it as CONTEXTS -- the text's
// edge, 0x0A, a word byte, any other byte -- and is a mask over the 16 pairs; in the NFA an epsilon edge that is open between two
// contexts of its mask.  The byte classes then refine the contexts.  A closure stops at an assertion; a subset in which one waits
// names the context of the byte it last took, and the assertion is resolved when the next byte is taken or the match ends: states
// multiply by at most the context count, under the same bound.  first[] holds one row per DISTINCT start row (contexts, at most 4;
// ctx_row[c] the row of context c in front of the start, row 0 the text edge's = the table's row 0), every terminal the contexts
// behind a match in which it accepts (acc_mask) and the lowest-numbered accepting expression for each (pat_ctx); the
// minimisation's first partition separates states by that whole record.  look_behind / look_ahead: some assertion depends on the
// context in front / behind.  A list without assertions compiles to the same plan whether they are admitted or not, with both 0.
// min_len, max_len and unbounded count consumed bytes.  A list that can match nowhere (a^b) is refused.
#ifndef BZH_REGEX_PLAN_H
#define BZH_REGEX_PLAN_H
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

enum : uint32_t {
    BZR_FOLD_ASCII = 1,
    BZR_DOTALL = 2,
    BZR_NO_LDS = 4,
    BZR_MAX_PATTERNS = 65536,
    BZR_MAX_EXPR = 4096,
    BZR_MAX_SPAN = 256,
    BZR_MAX_BOUND = 256,
    BZR_MAX_NEST = 256,
    BZR_MAX_NFA = 65536,
    BZR_MAX_STATES = 65535,
    BZR_LDS_ENTRIES = 2048, // a table of at most that many entries is staged into LDS by every workgroup (regex_core.h)
};
// the syntax word of bzr_compile_ex, apart from the flags: ASSERT admits ^ $ \A \Z \b \B; WORD and LINE wrap every expression
enum : uint32_t { BZR_SYN_ASSERT = 1, BZR_SYN_WORD = 2, BZR_SYN_LINE = 4 };
// THE CONTEXTS an assertion sees in front of and behind its place: the text's edge, 0x0A, a word byte [0-9A-Za-z_], any other byte
enum : uint32_t { BZR_CTX_EDGE = 0, BZR_CTX_NL = 1, BZR_CTX_WORD = 2, BZR_CTX_OTHER = 3, BZR_CONTEXTS = 4 };
static inline uint32_t bzr_ctx_of(uint32_t b) // of a byte (regex_core.h's bzr_ctx is the same rule on the device)
{
    if (b == '\n') return BZR_CTX_NL;
    return (b >= '0' && b <= '9') || (b >= 'A' && b <= 'Z') || (b >= 'a' && b <= 'z') || b == '_' ? BZR_CTX_WORD : BZR_CTX_OTHER;
}
// an assertion as the pairs (context in front, context behind) it holds for: bit 4 * front + behind
enum : uint8_t { BZR_AT_BOL, BZR_AT_EOL, BZR_AT_BOT, BZR_AT_EOT, BZR_AT_WORDB, BZR_AT_NWORDB, BZR_AT_NOWORD_FRONT, BZR_AT_NOWORD_BEHIND, BZR_AT_KINDS };
static const uint16_t BZR_AT_MASK[BZR_AT_KINDS] = {0x00FF, 0x3333, 0x000F, 0x1111, 0x4B44, 0xB4BB, 0xF0FF, 0xBBBB};

struct BzrPlan {
    uint64_t expressions = 0;
    uint32_t min_len = 0, max_len = 0, max_span = 0;
    uint32_t states = 0, classes = 0, nterm = 0; // rows and columns of the table, the terminal rows 1 .. nterm
    uint32_t unbounded = 0, in_lds = 0;
    uint32_t look_behind = 0, look_ahead = 0; // some assertion looks at the byte in front of a start / behind a match
    uint32_t contexts = 1;                    // distinct start rows: first[contexts * 256]
    uint8_t ctx_row[BZR_CONTEXTS] = {0, 0, 0, 0}; // the start row of a start whose front context is c
    uint8_t cls[256];
    uint16_t first[BZR_CONTEXTS * 256];
    std::vector<uint16_t> table;  // [states * classes]
    std::vector<uint32_t> pat_no; // [nterm]
    std::vector<uint8_t> acc_mask; // [nterm] with assertions: the contexts behind a match in which the terminal accepts, bit c
    std::vector<uint32_t> pat_ctx; // [nterm * 4] ... and the lowest-numbered expression that accepts there
    uint64_t table_bytes() const { return (uint64_t)table.size() * sizeof(uint16_t); }
};

struct BzrSet256 { // a set of byte values
    uint64_t w[4] = {0, 0, 0, 0};
    void add(uint32_t b) { w[b >> 6] |= 1ull << (b & 63); }
    void add_range(uint32_t lo, uint32_t hi)
    {
        for (uint32_t b = lo; b <= hi; b++) add(b);
    }
    bool has(uint32_t b) const { return (w[b >> 6] >> (b & 63)) & 1; }
    void join(const BzrSet256 &o)
    {
        for (int i = 0; i < 4; i++) w[i] |= o.w[i];
    }
    void invert()
    {
        for (int i = 0; i < 4; i++) w[i] = ~w[i];
    }
    bool none() const { return !(w[0] | w[1] | w[2] | w[3]); }
    void fold() // a letter brings its twin
    {
        for (uint32_t b = 'a'; b <= 'z'; b++)
            if (has(b) || has(b - 32)) add(b), add(b - 32);
    }
    bool operator<(const BzrSet256 &o) const { return memcmp(w, o.w, sizeof w) < 0; }
};

enum : uint8_t { BZR_N_SET, BZR_N_CAT, BZR_N_ALT, BZR_N_REP, BZR_N_LOOK };
enum : uint32_t { BZR_NONE = 0xFFFFFFFFu, BZR_INF = 0xFFFFFFFFu };
struct BzrNode {
    uint8_t kind;
    uint32_t set = 0;             // SET: its index; LOOK: its BZR_AT_ kind
    uint32_t lo = 0, hi = 0;      // REP: the bound (hi == BZR_INF: open)
    std::vector<uint32_t> kids;   // CAT, ALT: any number (a CAT of none matches the empty string); REP: one
};

// ---- the parser -------------------------------------------------------------------------------------------------------------------
struct BzrParser {
    const uint8_t *p;
    size_t n, expr;
    unsigned flags;
    char *err;
    size_t errn;
    std::vector<BzrNode> &nodes;
    std::vector<BzrSet256> &sets;
    std::map<BzrSet256, uint32_t> &set_ix;
    size_t i = 0;
    uint32_t nest = 0;
    bool bad = false;
    bool look = false;  // assertions are admitted
    uint32_t kinds = 0; // those met, bit BZR_AT_

    uint32_t fail(size_t at, const char *why)
    {
        if (!bad) snprintf(err, errn, "regex: expression %zu, byte %zu: %s", expr, at, why);
        bad = true;
        return BZR_NONE;
    }
    uint32_t node(BzrNode &&x)
    {
        nodes.push_back(std::move(x));
        return (uint32_t)nodes.size() - 1;
    }
    uint32_t set_node(BzrSet256 s)
    {
        auto it = set_ix.find(s);
        if (it == set_ix.end()) {
            sets.push_back(s);
            it = set_ix.emplace(s, (uint32_t)sets.size() - 1).first;
        }
        BzrNode x{BZR_N_SET, 0, 0, 0, {}};
        x.set = it->second;
        return node(std::move(x));
    }
    static int hexv(uint8_t c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; }
    // the escape at p[i] == '\\' into s; *multi: it is one of \d \D \w \W \s \S
    bool escape(BzrSet256 &s, bool *multi)
    {
        const size_t at = i;
        *multi = false;
        if (i + 1 >= n) return fail(at, "a backslash ends the expression"), false;
        const uint8_t c = p[i + 1];
        i += 2;
        switch (c) {
        case '\\': case '.': case '[': case ']': case '(': case ')': case '|': case '*': case '+': case '?': case '{': case '}': case '^':
        case '$': case '-': case '/':
            return s.add(c), true;
        case 'n': return s.add('\n'), true;
        case 't': return s.add('\t'), true;
        case 'r': return s.add('\r'), true;
        case 'f': return s.add('\f'), true;
        case 'v': return s.add('\v'), true;
        case '0':
            if (i < n && p[i] >= '0' && p[i] <= '9') return fail(at, "octal escapes are not supported"), false;
            return s.add(0), true;
        case 'x': {
            if (i + 2 > n || hexv(p[i]) < 0 || hexv(p[i + 1]) < 0) return fail(at, "\\x wants two hexadecimal digits"), false;
            s.add((uint32_t)(hexv(p[i]) * 16 + hexv(p[i + 1])));
            i += 2;
            return true;
        }
        case 'd': case 'D': case 'w': case 'W': case 's': case 'S': {
            BzrSet256 t;
            if (c == 'd' || c == 'D') t.add_range('0', '9');
            else if (c == 'w' || c == 'W') t.add_range('0', '9'), t.add_range('A', 'Z'), t.add_range('a', 'z'), t.add('_');
            else t.add(' '), t.add_range('\t', '\r');
            if (c < 'a') t.invert();
            s.join(t);
            *multi = true;
            return true;
        }
        default:
            if (c >= '1' && c <= '9') return fail(at, "backreferences are not supported"), false;
            if (c == 'b' || c == 'B' || c == 'A' || c == 'Z') return fail(at, "anchors and \\b are not supported"), false;
            if (c < 128 && !(c >= 'a' && c <= 'z') && !(c >= 'A' && c <= 'Z')) return s.add(c), true; // (as re takes what re.escape writes)
            return fail(at, "an escape that is not supported"), false;
        }
    }
    uint32_t look_node(uint32_t kind)
    {
        BzrNode x{BZR_N_LOOK, 0, 0, 0, {}};
        x.set = kind, kinds |= 1u << kind;
        return node(std::move(x));
    }
    uint32_t klass() // p[i] == '['
    {
        const size_t open = i++;
        bool neg = false;
        if (i < n && p[i] == '^') neg = true, i++;
        BzrSet256 s;
        bool first = true;
        for (;; first = false) {
            if (i >= n) return fail(open, "an unbalanced bracket: [ without ]");
            if (p[i] == ']' && !first) break;
            const size_t at = i;
            BzrSet256 one;
            bool multi = false;
            if (p[i] == '\\') {
                if (!escape(one, &multi)) return BZR_NONE;
            } else {
                one.add(p[i++]);
            }
            if (!multi && i + 1 < n && p[i] == '-' && p[i + 1] != ']') { // a range
                i++;
                BzrSet256 two;
                bool multi2 = false;
                if (p[i] == '\\') {
                    if (!escape(two, &multi2)) return BZR_NONE;
                } else {
                    two.add(p[i++]);
                }
                if (multi2) return fail(at, "a range that ends with a class escape");
                uint32_t lo = 0, hi = 0;
                while (!one.has(lo)) lo++;
                while (!two.has(hi)) hi++;
                if (hi < lo) return fail(at, "a range whose end lies in front of its start");
                s.add_range(lo, hi);
            } else {
                s.join(one);
            }
        }
        i++; // ]
        if (flags & BZR_FOLD_ASCII) s.fold();
        if (neg) s.invert();
        return set_node(s);
    }
    uint32_t atom()
    {
        const size_t at = i;
        const uint8_t c = p[i];
        if (c == '(') {
            i++;
            if (i < n && p[i] == '?') {
                if (i + 1 < n && p[i + 1] == ':') i += 2;
                else return fail(at, "lookaround, named groups and inline flags are not supported");
            }
            if (++nest > BZR_MAX_NEST) return fail(at, "groups nested deeper than 256");
            const uint32_t r = alt();
            nest--;
            if (bad) return BZR_NONE;
            if (i >= n || p[i] != ')') return fail(at, "an unbalanced bracket: ( without )");
            i++;
            return r;
        }
        if (c == '[') return klass();
        if ((c == '^' || c == '$') && look) return i++, look_node(c == '^' ? BZR_AT_BOL : BZR_AT_EOL);
        if (c == '^' || c == '$') return fail(at, "anchors are not supported");
        if (c == '*' || c == '+' || c == '?') return fail(at, "a quantifier with nothing to repeat");
        if (c == '{') return fail(at, "a { that opens no well-formed bound");
        BzrSet256 s;
        if (c == '.') {
            i++;
            s.invert();
            if (!(flags & BZR_DOTALL)) s.w[0] &= ~(1ull << '\n');
            return set_node(s);
        }
        if (c == '\\') {
            if (look && i + 1 < n && (p[i + 1] == 'b' || p[i + 1] == 'B' || p[i + 1] == 'A' || p[i + 1] == 'Z')) {
                const uint8_t e = p[i + 1];
                i += 2;
                return look_node(e == 'b' ? BZR_AT_WORDB : e == 'B' ? BZR_AT_NWORDB : e == 'A' ? BZR_AT_BOT : BZR_AT_EOT);
            }
            bool multi;
            if (!escape(s, &multi)) return BZR_NONE;
        } else {
            s.add(c), i++;
        }
        if (flags & BZR_FOLD_ASCII) s.fold();
        return set_node(s);
    }
    bool number(uint32_t *v) // digits at p[i]
    {
        if (i >= n || p[i] < '0' || p[i] > '9') return false;
        uint32_t x = 0;
        while (i < n && p[i] >= '0' && p[i] <= '9') x = x > 100000 ? x : x * 10 + (p[i] - '0'), i++;
        *v = x;
        return true;
    }
    uint32_t repeat()
    {
        uint32_t a = atom();
        if (bad) return BZR_NONE;
        if (i >= n) return a;
        const size_t at = i;
        uint32_t lo, hi;
        const uint8_t c = p[i];
        if (c == '?') lo = 0, hi = 1, i++;
        else if (c == '*') lo = 0, hi = BZR_INF, i++;
        else if (c == '+') lo = 1, hi = BZR_INF, i++;
        else if (c == '{') {
            i++;
            if (!number(&lo)) return fail(at, "a { that opens no well-formed bound");
            hi = lo;
            if (i < n && p[i] == ',') {
                i++;
                if (!number(&hi)) hi = BZR_INF;
            }
            if (i >= n || p[i] != '}') return fail(at, "a { that opens no well-formed bound");
            i++;
            if (lo > BZR_MAX_BOUND || (hi != BZR_INF && hi > BZR_MAX_BOUND)) return fail(at, "a bound above 256");
            if (hi < lo) return fail(at, "a bound whose maximum lies below its minimum");
        } else {
            return a;
        }
        if (nodes[a].kind == BZR_N_LOOK && p[at - 1] != ')') return fail(at, "a quantifier with nothing to repeat"); // (as re: an assertion is nothing to repeat)
        if (i < n && (p[i] == '?' || p[i] == '+')) return fail(i, "lazy and possessive quantifiers are not supported");
        if (i < n && (p[i] == '*' || p[i] == '{')) return fail(i, "a quantifier behind a quantifier");
        BzrNode x{BZR_N_REP, 0, 0, 0, {}};
        x.lo = lo, x.hi = hi, x.kids.push_back(a);
        return node(std::move(x));
    }
    uint32_t cat()
    {
        BzrNode x{BZR_N_CAT, 0, 0, 0, {}};
        while (i < n && p[i] != '|' && p[i] != ')') {
            const uint32_t r = repeat();
            if (bad) return BZR_NONE;
            x.kids.push_back(r);
        }
        if (x.kids.size() == 1) return x.kids[0];
        return node(std::move(x));
    }
    uint32_t alt()
    {
        BzrNode x{BZR_N_ALT, 0, 0, 0, {}};
        for (;;) {
            const uint32_t r = cat();
            if (bad) return BZR_NONE;
            x.kids.push_back(r);
            if (i < n && p[i] == '|') i++;
            else break;
        }
        if (x.kids.size() == 1) return x.kids[0];
        return node(std::move(x));
    }
    uint32_t top()
    {
        const uint32_t r = alt();
        if (bad) return BZR_NONE;
        if (i < n) return fail(i, "an unbalanced bracket: ) without ("); // (only a ')' stops alt() early)
        return r;
    }
};

// the shortest match of a node, saturating
static inline uint64_t bzr_min_len(const std::vector<BzrNode> &nodes, const std::vector<BzrSet256> &sets, uint32_t v)
{
    const uint64_t cap = 1u << 30;
    const BzrNode &x = nodes[v];
    uint64_t r = 0;
    switch (x.kind) {
    case BZR_N_SET: return sets[x.set].none() ? cap : 1;
    case BZR_N_LOOK: return 0;
    case BZR_N_CAT:
        for (uint32_t k : x.kids) r = std::min(cap, r + bzr_min_len(nodes, sets, k));
        return r;
    case BZR_N_ALT:
        r = cap;
        for (uint32_t k : x.kids) r = std::min(r, bzr_min_len(nodes, sets, k));
        return r;
    default: return std::min(cap, (uint64_t)x.lo * bzr_min_len(nodes, sets, x.kids[0]));
    }
}

// ---- the NFA ----------------------------------------------------------------------------------------------------------------------
struct BzrNfa {
    struct St {
        int32_t set;     // >= 0: takes a byte of that set to `e1`; -1: the edges e1, e2 take nothing; -2: e1 takes nothing and is
        uint32_t e1, e2; // open only between two contexts of `mask`
        uint16_t mask;
    };
    std::vector<St> st;
    std::vector<int32_t> accept; // the expression that accepts in a state, or -1
    uint32_t positions = 0;
    bool over = false;
    const std::vector<BzrNode> *nodes = nullptr;

    uint32_t add(int32_t set)
    {
        if (st.size() >= 8u * BZR_MAX_NFA) over = true;
        st.push_back(St{set, BZR_NONE, BZR_NONE, 0});
        return (uint32_t)st.size() - 1;
    }
    void edge(uint32_t from, uint32_t to)
    {
        if (st[from].e1 == BZR_NONE) st[from].e1 = to;
        else st[from].e2 = to;
    }
    // the fragment of node v: *s its entry, *e its exit, a state without edges
    void build(uint32_t v, uint32_t *s, uint32_t *e)
    {
        if (over) {
            *s = *e = 0;
            return;
        }
        const BzrNode &x = (*nodes)[v];
        switch (x.kind) {
        case BZR_N_SET:
            if (++positions > BZR_MAX_NFA) over = true;
            *s = add((int32_t)x.set), *e = add(-1);
            st[*s].e1 = *e;
            return;
        case BZR_N_LOOK:
            *s = add(-2), *e = add(-1);
            st[*s].e1 = *e, st[*s].mask = BZR_AT_MASK[x.set];
            return;
        case BZR_N_CAT: {
            *s = *e = add(-1);
            for (uint32_t k : x.kids) {
                uint32_t ks, ke;
                build(k, &ks, &ke);
                if (over) return;
                edge(*e, ks), *e = ke;
            }
            return;
        }
        case BZR_N_ALT: {
            uint32_t split = add(-1);
            *s = split, *e = add(-1);
            for (size_t j = 0; j < x.kids.size(); j++) {
                uint32_t ks, ke;
                build(x.kids[j], &ks, &ke);
                if (over) return;
                edge(split, ks), edge(ke, *e);
                if (j + 2 < x.kids.size()) { // (two edges a state: a chain of splits)
                    const uint32_t next = add(-1);
                    edge(split, next), split = next;
                }
            }
            return;
        }
        default: {
            *s = *e = add(-1);
            for (uint32_t r = 0; r < x.lo && !over; r++) {
                uint32_t ks, ke;
                build(x.kids[0], &ks, &ke);
                if (over) return;
                edge(*e, ks), *e = ke;
            }
            if (x.hi == BZR_INF) { // x*: loop -> x -> loop, loop -> out
                uint32_t ks, ke;
                const uint32_t loop = add(-1), out = add(-1);
                build(x.kids[0], &ks, &ke);
                if (over) return;
                edge(*e, loop), edge(loop, ks), edge(loop, out), edge(ke, loop);
                *e = out;
            } else if (x.hi > x.lo) { // (x(x(x)?)?)?: every copy may be left out, and those behind it with it
                const uint32_t out = add(-1);
                for (uint32_t r = x.lo; r < x.hi && !over; r++) {
                    uint32_t ks, ke;
                    const uint32_t opt = add(-1);
                    build(x.kids[0], &ks, &ke);
                    if (over) return;
                    edge(*e, opt), edge(opt, ks), edge(opt, out), *e = ke;
                }
                edge(*e, out), *e = out;
            }
            return;
        }
        }
    }
};

// Compiles exprs[0 .. count) into `out`.  max_span: 1 .. 256, 0 = 256.  syntax: BZR_SYN_*.  Returns true, or false with the reason
// in err[0 .. errn).  A list that holds no assertion compiles to the same plan whatever `syntax` admits.
static inline bool bzr_compile_ex(const uint8_t *const *exprs, const size_t *lens, size_t count, unsigned flags, uint32_t max_span, unsigned syntax,
                                  BzrPlan &out, char *err, size_t errn)
{
    if (syntax & ~(unsigned)(BZR_SYN_ASSERT | BZR_SYN_WORD | BZR_SYN_LINE)) return snprintf(err, errn, "regex: syntax 0x%x, of which only 0x7 are defined", syntax), false;
    if ((syntax & BZR_SYN_WORD) && (syntax & BZR_SYN_LINE)) return snprintf(err, errn, "regex: the word wrap and the line wrap exclude each other"), false;
    if (count == 0 || count > BZR_MAX_PATTERNS) return snprintf(err, errn, "regex: %zu expressions, outside 1..%u", count, (unsigned)BZR_MAX_PATTERNS), false;
    if (!exprs || !lens) return snprintf(err, errn, "regex: a null array"), false;
    if (flags & ~(unsigned)(BZR_FOLD_ASCII | BZR_DOTALL | BZR_NO_LDS)) return snprintf(err, errn, "regex: flags 0x%x, of which only 0x7 are defined", flags), false;
    if (max_span > BZR_MAX_SPAN) return snprintf(err, errn, "regex: max_span %u, outside 0..%u", max_span, (unsigned)BZR_MAX_SPAN), false;
    if (max_span == 0) max_span = BZR_MAX_SPAN;
    for (size_t i = 0; i < count; i++) {
        if (lens[i] == 0 || lens[i] > BZR_MAX_EXPR) return snprintf(err, errn, "regex: expression %zu, byte 0: it has %zu bytes, outside 1..%u", i, lens[i], (unsigned)BZR_MAX_EXPR), false;
        if (!exprs[i]) return snprintf(err, errn, "regex: expression %zu, byte 0: it is null", i), false;
    }

    // parse
    std::vector<BzrNode> nodes;
    std::vector<BzrSet256> sets;
    std::map<BzrSet256, uint32_t> set_ix;
    std::vector<uint32_t> roots(count);
    uint32_t kinds = 0; // the assertions met
    for (size_t i = 0; i < count; i++) {
        BzrParser ps{exprs[i], lens[i], i, flags, err, errn, nodes, sets, set_ix};
        ps.look = (syntax & BZR_SYN_ASSERT) != 0;
        roots[i] = ps.top();
        if (ps.bad) return false;
        kinds |= ps.kinds;
        if (syntax & (BZR_SYN_WORD | BZR_SYN_LINE)) { // the wrap: an assertion, the expression, an assertion
            const bool word = (syntax & BZR_SYN_WORD) != 0;
            const uint32_t a = ps.look_node(word ? BZR_AT_NOWORD_FRONT : BZR_AT_BOL), b = ps.look_node(word ? BZR_AT_NOWORD_BEHIND : BZR_AT_EOL);
            BzrNode x{BZR_N_CAT, 0, 0, 0, {a, roots[i], b}};
            roots[i] = ps.node(std::move(x));
            kinds |= ps.kinds;
        }
        const uint64_t mn = bzr_min_len(nodes, sets, roots[i]);
        if (mn == 0) return snprintf(err, errn, "regex: expression %zu, byte 0: it matches the empty string", i), false;
        if (mn > max_span) return snprintf(err, errn, "regex: expression %zu, byte 0: its shortest match exceeds max_span %u", i, max_span), false;
    }

    // the NFA: state 0 and a chain of splits lead to every expression's fragment
    BzrNfa nfa;
    nfa.nodes = &nodes;
    uint32_t split = nfa.add(-1);
    std::vector<std::pair<uint32_t, uint32_t>> ends;
    for (size_t i = 0; i < count; i++) {
        uint32_t s, e;
        nfa.build(roots[i], &s, &e);
        if (nfa.over) return snprintf(err, errn, "regex: expression %zu, byte 0: the NFA exceeds %u positions behind the expansion of its repeats", i, (unsigned)BZR_MAX_NFA), false;
        nfa.edge(split, s);
        ends.emplace_back(e, (uint32_t)i);
        if (i + 1 < count) {
            const uint32_t next = nfa.add(-1);
            nfa.edge(split, next), split = next;
        }
    }
    nfa.accept.assign(nfa.st.size(), -1);
    for (auto &pe : ends) nfa.accept[pe.first] = (int32_t)pe.second;

    // the classes: bytes that lie in the same sets
    const bool looks = kinds != 0;
    for (uint32_t k = 0; k < BZR_AT_KINDS; k++)
        if (kinds >> k & 1u) {
            const uint16_t m = BZR_AT_MASK[k];
            for (uint32_t c = 0; c < BZR_CONTEXTS; c++) {
                if ((m >> (4 * c) & 15u) != (m & 15u)) out.look_behind = 1;
                if ((m >> (4 * c) & 15u) != 0 && (m >> (4 * c) & 15u) != 15u) out.look_ahead = 1;
            }
        }
    uint32_t tmp[256] = {};
    uint32_t ncls = 1;
    std::vector<BzrSet256> splits(sets); // with assertions the classes refine the contexts as well
    if (looks) {
        BzrSet256 nl, word;
        for (uint32_t b = 0; b < 256; b++)
            if (bzr_ctx_of(b) == BZR_CTX_NL) nl.add(b);
            else if (bzr_ctx_of(b) == BZR_CTX_WORD) word.add(b);
        splits.push_back(nl), splits.push_back(word);
    }
    for (const BzrSet256 &s : splits) {
        std::map<std::pair<uint32_t, bool>, uint32_t> split_ix;
        uint32_t next = 0;
        for (uint32_t b = 0; b < 256; b++) {
            auto it = split_ix.emplace(std::make_pair(tmp[b], s.has(b)), next);
            if (it.second) next++;
            tmp[b] = it.first->second;
        }
        ncls = next;
    }
    BzrSet256 any;
    for (const BzrSet256 &s : sets) any.join(s);
    {
        int32_t renum[256];
        for (uint32_t c = 0; c < 256; c++) renum[c] = -1;
        uint32_t next = 0;
        for (uint32_t b = 0; b < 256; b++)
            if (!any.has(b)) renum[tmp[b]] = 0, next = 1; // the dead class, if there is one
        for (uint32_t b = 0; b < 256; b++) {
            if (renum[tmp[b]] < 0) renum[tmp[b]] = (int32_t)next++;
            out.cls[b] = (uint8_t)renum[tmp[b]];
        }
        ncls = next;
    }
    const uint32_t dead_cls = any.w[0] == ~0ull && any.w[1] == ~0ull && any.w[2] == ~0ull && any.w[3] == ~0ull ? (uint32_t)BZR_NONE : 0u;
    uint32_t rep[256]; // a byte of every class
    for (uint32_t b = 256; b-- > 0;) rep[out.cls[b]] = b;

    // subset construction: a subset is the sorted list of its states that take a byte or accept
    std::vector<uint32_t> stamp(nfa.st.size(), 0), stack, cur;
    uint32_t tick = 0;
    auto closure_add = [&](uint32_t from) {
        stack.push_back(from);
        while (!stack.empty()) {
            const uint32_t v = stack.back();
            stack.pop_back();
            if (stamp[v] == tick) continue;
            stamp[v] = tick;
            const BzrNfa::St &x = nfa.st[v];
            if (x.set >= 0 || x.set == -2 || nfa.accept[v] >= 0) cur.push_back(v); // (an assertion stops the closure: its contexts are not known yet)
            if (x.set == -1) {
                if (x.e1 != BZR_NONE) stack.push_back(x.e1);
                if (x.e2 != BZR_NONE) stack.push_back(x.e2);
            }
        }
    };
    // WITH ASSERTIONS a subset that holds one also names the context of the byte it last took (its last element, BZR_TAG | context):
    // the assertion is resolved when the next byte is taken, or the match ends, and both contexts are known.  `open`: the states of
    // a subset that take a byte or accept between the contexts pc and nc -- the subset itself, and what lies behind its assertions
    // that hold there.  Without assertions open() is the subset, and everything below is what it was.
    const uint32_t BZR_TAG = 0xFFFFFFF0u;
    std::vector<uint32_t> stamp2(looks ? nfa.st.size() : 0, 0), ex;
    uint32_t tick2 = 0;
    auto tag_of = [&](const std::vector<uint32_t> &sub) { return !sub.empty() && sub.back() >= BZR_TAG ? sub.back() - BZR_TAG : 0u; };
    auto open = [&](const std::vector<uint32_t> &sub, uint32_t pc, uint32_t nc) -> const std::vector<uint32_t> & {
        if (!looks || sub.empty() || sub.back() < BZR_TAG) return sub;
        ex.clear(), tick2++;
        std::vector<uint32_t> todo(sub.begin(), sub.end() - 1);
        while (!todo.empty()) {
            const uint32_t v = todo.back();
            todo.pop_back();
            if (stamp2[v] == tick2) continue;
            stamp2[v] = tick2;
            const BzrNfa::St &x = nfa.st[v];
            if (x.set == -2) {
                if (x.mask >> (4 * pc + nc) & 1u) todo.push_back(x.e1);
            } else if (x.set == -1) {
                if (nfa.accept[v] >= 0) ex.push_back(v);
                if (x.e1 != BZR_NONE) todo.push_back(x.e1);
                if (x.e2 != BZR_NONE) todo.push_back(x.e2);
            } else {
                ex.push_back(v);
            }
        }
        return ex;
    };
    auto seal = [&](uint32_t pc) { // cur, sorted, and the context it was entered from if an assertion waits in it
        std::sort(cur.begin(), cur.end());
        bool waits = false;
        for (uint32_t v : cur) waits = waits || nfa.st[v].set == -2;
        if (waits) cur.push_back(BZR_TAG + pc);
    };
    std::vector<std::vector<uint32_t>> subset;
    std::map<std::vector<uint32_t>, uint32_t> subset_ix; // (the roots are not in it: where a root's subset recurs it gets a row of its own)
    std::vector<uint32_t> trans;                          // [states * ncls], 0 = dead
    std::vector<int32_t> acc;                             // the lowest expression that accepts, behind whichever context
    std::vector<uint32_t> accid;                          // ... and the number of the whole record, one expression a context
    std::vector<std::array<int32_t, BZR_CONTEXTS>> acc4;
    std::map<std::array<int32_t, BZR_CONTEXTS>, uint32_t> acc_ix;
    std::vector<uint32_t> depth_of; // breadth-first: a subset's number ascends with its depth
    bool cut = false;               // a row max_span deep has a live transition: no walk takes it, so it is left dead
    tick++, cur.clear(), closure_add(0);
    seal(0);
    const uint32_t NR = cur.back() >= BZR_TAG ? (uint32_t)BZR_CONTEXTS : 1u; // the roots: one a context in front of the start, if it is looked at
    for (uint32_t r = 0; r < NR; r++) {
        if (NR > 1) cur.back() = BZR_TAG + r;
        subset.push_back(cur), depth_of.push_back(0);
    }
    uint32_t ctx_cls[256]; // the context of a class's bytes (with assertions the classes refine them)
    for (uint32_t c = 0; c < ncls; c++) ctx_cls[c] = looks ? bzr_ctx_of(rep[c]) : 0u;
    for (uint32_t d = 0; d < subset.size(); d++) {
        const uint32_t pc = tag_of(subset[d]);
        std::array<int32_t, BZR_CONTEXTS> a4;
        int32_t a = -1;
        for (uint32_t nc = 0; nc < BZR_CONTEXTS; nc++) {
            a4[nc] = -1;
            for (uint32_t v : open(subset[d], pc, nc))
                if (nfa.accept[v] >= 0 && (a4[nc] < 0 || nfa.accept[v] < a4[nc])) a4[nc] = nfa.accept[v];
            if (a4[nc] >= 0 && (a < 0 || a4[nc] < a)) a = a4[nc];
        }
        acc.push_back(a), acc4.push_back(a4);
        accid.push_back(acc_ix.emplace(a4, (uint32_t)acc_ix.size()).first->second);
        trans.resize((size_t)(d + 1) * ncls, 0);
        for (uint32_t c = 0; c < ncls; c++) {
            if (c == dead_cls) continue;
            const std::vector<uint32_t> &from = open(subset[d], pc, ctx_cls[c]); // (read before subset grows below)
            if (depth_of[d] >= max_span) {
                for (uint32_t v : from) cut = cut || (nfa.st[v].set >= 0 && sets[nfa.st[v].set].has(rep[c]));
                continue;
            }
            tick++, cur.clear();
            for (uint32_t v : from) {
                const BzrNfa::St &x = nfa.st[v];
                if (x.set >= 0 && sets[x.set].has(rep[c])) closure_add(x.e1);
            }
            if (cur.empty()) continue;
            seal(ctx_cls[c]);
            auto it = subset_ix.find(cur);
            if (it == subset_ix.end()) {
                if (subset.size() > BZR_MAX_STATES)
                    return snprintf(err, errn, "regex: the automaton needs more than %u states beyond the root", (unsigned)BZR_MAX_STATES), false;
                it = subset_ix.emplace(cur, (uint32_t)subset.size()).first;
                subset.push_back(cur);
                depth_of.push_back(depth_of[d] + 1);
            }
            trans[(size_t)d * ncls + c] = it->second;
        }
    }
    const uint32_t S = (uint32_t)subset.size();
    subset.clear(), subset_ix.clear();

    // minimisation.  Block 0 holds the dead state and every state that reaches no terminal; the root stands outside -- nothing leads
    // to it.  The states that reach no cycle are peeled off from the leaves up, each named by its terminal and the blocks behind its
    // transitions -- one pass, which is all a list of words needs; the rest, usually a handful, is refined round by round (Moore),
    // first by the lowest expression that accepts.
    std::vector<uint32_t> block(S, 0);
    uint32_t nblocks = 1;
    {
        std::vector<uint32_t> pstart(S + 1, 0), pred; // the transitions backwards, one entry an edge
        for (size_t e = 0; e < trans.size(); e++)
            if (trans[e]) pstart[trans[e] + 1]++;
        for (uint32_t s = 0; s < S; s++) pstart[s + 1] += pstart[s];
        pred.resize(pstart[S]);
        {
            std::vector<uint32_t> fill(pstart.begin(), pstart.end() - 1);
            for (uint32_t s = 0; s < S; s++)
                for (uint32_t c = 0; c < ncls; c++)
                    if (trans[(size_t)s * ncls + c]) pred[fill[trans[(size_t)s * ncls + c]]++] = s;
        }
        std::vector<uint8_t> live(S, 0); // reaches a terminal
        std::vector<uint32_t> work;
        for (uint32_t s = 0; s < S; s++)
            if (acc[s] >= 0) live[s] = 1, work.push_back(s);
        while (!work.empty()) {
            const uint32_t s = work.back();
            work.pop_back();
            for (uint32_t e = pstart[s]; e < pstart[s + 1]; e++)
                if (!live[pred[e]]) live[pred[e]] = 1, work.push_back(pred[e]);
        }
        for (size_t e = 0; e < trans.size(); e++)
            if (trans[e] && !live[trans[e]]) trans[e] = 0;
        std::vector<uint32_t> outdeg(S, 0);
        for (uint32_t s = 0; s < S; s++)
            for (uint32_t c = 0; c < ncls; c++) outdeg[s] += trans[(size_t)s * ncls + c] != 0;
        for (uint32_t s = 0; s < S; s++)
            if (live[s] && !outdeg[s]) work.push_back(s);
        std::unordered_map<std::string, uint32_t> sig_ix;
        std::vector<uint32_t> sig(ncls + 1, 0);
        std::vector<uint8_t> peeled(S, 0);
        auto key = [&]() { return std::string(reinterpret_cast<const char *>(sig.data()), sig.size() * 4); };
        while (!work.empty()) {
            const uint32_t s = work.back();
            work.pop_back();
            peeled[s] = 1;
            if (s >= NR) { // (every state behind its transitions has its block)
                sig[0] = accid[s] + 1;
                for (uint32_t c = 0; c < ncls; c++) sig[c + 1] = trans[(size_t)s * ncls + c] ? block[trans[(size_t)s * ncls + c]] : 0u;
                block[s] = sig_ix.emplace(key(), (uint32_t)sig_ix.size() + 1).first->second;
            }
            for (uint32_t e = pstart[s]; e < pstart[s + 1]; e++)
                if (live[pred[e]] && --outdeg[pred[e]] == 0) work.push_back(pred[e]);
        }
        const uint32_t fixed = (uint32_t)sig_ix.size() + 1; // blocks [0, fixed) stand
        std::vector<uint32_t> rest;
        for (uint32_t s = NR; s < S; s++)
            if (live[s] && !peeled[s]) rest.push_back(s);
        nblocks = fixed;
        if (!rest.empty()) {
            std::map<uint32_t, uint32_t> by_acc;
            for (uint32_t s : rest) block[s] = fixed + by_acc.emplace(accid[s], (uint32_t)by_acc.size()).first->second;
            uint32_t parts = (uint32_t)by_acc.size();
            std::vector<uint32_t> nb(rest.size());
            for (;;) {
                sig_ix.clear();
                for (size_t j = 0; j < rest.size(); j++) {
                    const uint32_t s = rest[j];
                    sig[0] = block[s];
                    for (uint32_t c = 0; c < ncls; c++) sig[c + 1] = trans[(size_t)s * ncls + c] ? block[trans[(size_t)s * ncls + c]] : 0u;
                    nb[j] = fixed + sig_ix.emplace(key(), (uint32_t)sig_ix.size()).first->second;
                }
                for (size_t j = 0; j < rest.size(); j++) block[rest[j]] = nb[j];
                const uint32_t now = (uint32_t)sig_ix.size();
                if (now == parts) break;
                parts = now;
            }
            nblocks = fixed + parts;
        }
    }
    // the rows: the root, and a member of every block but 0; numbered in breadth-first order, the terminals first
    std::vector<uint32_t> member(nblocks, BZR_NONE);
    for (uint32_t s = S; s-- > NR;) member[block[s]] = s;
    auto target = [&](uint32_t s, uint32_t c) { // the block behind a transition; 0: dead
        const uint32_t t = trans[(size_t)s * ncls + c];
        return t ? block[t] : 0u;
    };
    std::vector<uint32_t> order, seen(nblocks, 0); // blocks in breadth-first order from the root
    {
        size_t head = 0;
        for (uint32_t r = 0; r < NR; r++)
            for (uint32_t c = 0; c < ncls; c++) {
                const uint32_t b = target(r, c);
                if (b && !seen[b]) seen[b] = 1, order.push_back(b);
            }
        while (head < order.size()) {
            const uint32_t s = member[order[head++]];
            for (uint32_t c = 0; c < ncls; c++) {
                const uint32_t b = target(s, c);
                if (b && !seen[b]) seen[b] = 1, order.push_back(b);
            }
        }
    }
    std::vector<uint32_t> num(nblocks, 0);
    uint32_t nterm = 0, next = 0;
    for (uint32_t b : order)
        if (acc[member[b]] >= 0) nterm++;
    if (nterm == 0) return snprintf(err, errn, "regex: no expression can match anywhere: its assertions contradict each other"), false; // (a^b)
    out.pat_no.assign(nterm, 0);
    next = nterm;
    {
        uint32_t t = 0;
        for (uint32_t b : order) {
            if (acc[member[b]] >= 0) num[b] = ++t, out.pat_no[t - 1] = (uint32_t)acc[member[b]];
            else num[b] = ++next;
        }
    }
    out.states = (uint32_t)order.size() + 1;
    out.classes = ncls;
    out.nterm = nterm;
    out.table.assign((size_t)out.states * ncls, 0);
    for (uint32_t c = 0; c < ncls; c++) out.table[c] = (uint16_t)num[target(0, c)];
    for (uint32_t b : order)
        for (uint32_t c = 0; c < ncls; c++) out.table[(size_t)num[b] * ncls + c] = (uint16_t)num[target(member[b], c)];
    for (uint32_t b = 0; b < 256; b++) out.first[b] = out.table[out.cls[b]];
    // the start rows: one a context in front of the start, equal ones merged; row 0 is the text edge's and the table's row 0
    out.contexts = 1;
    std::vector<uint16_t> extra; // the rows of the further roots, as the table would hold them
    for (uint32_t r = 1; r < NR; r++) {
        uint16_t row[256];
        for (uint32_t b = 0; b < 256; b++) row[b] = (uint16_t)num[target(r, out.cls[b])];
        uint32_t same = 0;
        while (same < out.contexts && memcmp(out.first + 256 * same, row, sizeof row)) same++;
        out.ctx_row[r] = (uint8_t)same;
        if (same < out.contexts) continue;
        memcpy(out.first + 256 * out.contexts++, row, sizeof row);
        for (uint32_t c = 0; c < ncls; c++) extra.push_back((uint16_t)num[target(r, c)]);
    }
    for (uint32_t r = out.contexts; r < BZR_CONTEXTS; r++) memset(out.first + 256 * r, 0, 512);
    if (looks) { // what a terminal accepts behind every context
        out.acc_mask.assign(nterm, 0), out.pat_ctx.assign((size_t)nterm * BZR_CONTEXTS, 0);
        for (uint32_t b : order)
            if (num[b] <= nterm)
                for (uint32_t c = 0; c < BZR_CONTEXTS; c++)
                    if (acc4[member[b]][c] >= 0) out.acc_mask[num[b] - 1] |= (uint8_t)(1u << c), out.pat_ctx[(size_t)(num[b] - 1) * BZR_CONTEXTS + c] = (uint32_t)acc4[member[b]][c];
    }

    // min_len: breadth-first depth of the first terminal; the longest match: a topological order of the rows (every row lies on a
    // path to a terminal), which a cycle leaves incomplete
    // (the further start rows stand behind the table's for this)
    std::vector<uint16_t> all(out.table);
    all.insert(all.end(), extra.begin(), extra.end());
    const uint32_t R = (uint32_t)(all.size() / ncls);
    {
        std::vector<uint32_t> depth(R, BZR_NONE), q{0};
        depth[0] = 0;
        for (uint32_t r = out.states; r < R; r++) depth[r] = 0, q.push_back(r);
        out.min_len = 0;
        for (size_t h = 0; h < q.size() && !out.min_len; h++)
            for (uint32_t c = 0; c < ncls; c++) {
                const uint32_t t = all[(size_t)q[h] * ncls + c];
                if (!t || depth[t] != BZR_NONE) continue;
                depth[t] = depth[q[h]] + 1;
                if (t <= nterm) {
                    out.min_len = depth[t];
                    break;
                }
                q.push_back(t);
            }
        std::vector<uint32_t> indeg(R, 0), longest(R, 0), ready{0};
        for (uint32_t r = out.states; r < R; r++) ready.push_back(r);
        for (size_t e = 0; e < all.size(); e++)
            if (all[e]) indeg[all[e]]++;
        uint32_t done = 0, far = 0;
        while (!ready.empty()) {
            const uint32_t s = ready.back();
            ready.pop_back();
            done++;
            if (s && s <= nterm) far = std::max(far, longest[s]);
            for (uint32_t c = 0; c < ncls; c++) {
                const uint32_t t = all[(size_t)s * ncls + c];
                if (!t) continue;
                longest[t] = std::max(longest[t], longest[s] + 1);
                if (--indeg[t] == 0) ready.push_back(t);
            }
        }
        out.unbounded = cut || done < R || far > max_span;
        out.max_len = out.unbounded ? max_span : far;
    }
    out.expressions = count;
    out.max_span = max_span;
    out.in_lds = !(flags & BZR_NO_LDS) && out.table.size() <= BZR_LDS_ENTRIES;
    return true;
}

static inline bool bzr_compile(const uint8_t *const *exprs, const size_t *lens, size_t count, unsigned flags, uint32_t max_span, BzrPlan &out,
                               char *err, size_t errn)
{
    return bzr_compile_ex(exprs, lens, count, flags, max_span, 0, out, err, errn);
}

#endif // BZH_REGEX_PLAN_H
