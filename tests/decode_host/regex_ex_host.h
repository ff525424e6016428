// regex_ex_host.h -- the harnesses' OWN regular expressions, shared by regex_host.cpp and look_host.cpp: a tree, its text for the
// compiler of banzai_amd/csrc/regex_plan.h, and the naive matcher on the tree -- no table, no automaton in it.  A tree without a
// LOOK node is an expression without assertions; `n`, the text's end, matters to LOOK nodes alone.
#ifndef BZH_REGEX_EX_HOST_H
#define BZH_REGEX_EX_HOST_H
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <bitset>
#include <set>
#include <string>
#include <vector>

struct Ex {
    enum Kind { SET, CAT, ALT, REP, LOOK } kind = SET;
    std::bitset<256> set;
    bool neg = false;
    std::string text;     // SET, LOOK: how it is written
    char look = 0;        // LOOK: ^ $ A Z b B, and < > for the word wrap's two ends
    std::vector<Ex> kids;
    uint32_t lo = 0, hi = 0;
};
static inline uint8_t twin(uint8_t b) { return b >= 'A' && b <= 'Z' ? (uint8_t)(b + 32) : b >= 'a' && b <= 'z' ? (uint8_t)(b - 32) : b; }
static inline bool takes(const Ex &e, uint8_t b, bool fold) { return (e.set[b] || (fold && e.set[twin(b)])) != e.neg; }
static inline bool wordb(uint8_t b) { return (b >= '0' && b <= '9') || (b >= 'a' && b <= 'z') || (b >= 'A' && b <= 'Z') || b == '_'; }
// THE RULE of an assertion at position p of t[0, n), by its words and not by the contexts
static inline bool holds(char look, const uint8_t *t, uint64_t n, uint64_t p)
{
    const bool wf = p > 0 && wordb(t[p - 1]), wb = p < n && wordb(t[p]);
    switch (look) {
    case '^': return p == 0 || t[p - 1] == '\n';
    case '$': return p == n || t[p] == '\n';
    case 'A': return p == 0;
    case 'Z': return p == n;
    case 'b': return wf != wb;
    case 'B': return wf == wb;
    case '<': return !wf;
    default: return !wb;
    }
}
typedef std::set<uint64_t> Ends;
// the positions behind a match of e that begins at one of `in`, no byte at or behind lim taken; the text is t[0, n)
static inline Ends ends(const Ex &e, const uint8_t *t, uint64_t n, uint64_t lim, const Ends &in, bool fold)
{
    Ends out;
    switch (e.kind) {
    case Ex::SET:
        for (uint64_t p : in)
            if (p < lim && takes(e, t[p], fold)) out.insert(p + 1);
        return out;
    case Ex::LOOK:
        for (uint64_t p : in)
            if (holds(e.look, t, n, p)) out.insert(p);
        return out;
    case Ex::CAT:
        out = in;
        for (const Ex &k : e.kids) out = ends(k, t, n, lim, out, fold);
        return out;
    case Ex::ALT:
        for (const Ex &k : e.kids) {
            const Ends x = ends(k, t, n, lim, in, fold);
            out.insert(x.begin(), x.end());
        }
        return out;
    default: {
        Ends cur = in;
        if (e.lo == 0) out = in;
        for (uint32_t k = 1; e.hi == ~0u || k <= e.hi; k++) {
            cur = ends(e.kids[0], t, n, lim, cur, fold);
            if (cur.empty()) break;
            if (k < e.lo) continue;
            const size_t before = out.size();
            out.insert(cur.begin(), cur.end());
            if (out.size() == before && k > e.lo) break;
        }
        return out;
    }
    }
}
static inline uint64_t min_len(const Ex &e)
{
    uint64_t r = 0;
    switch (e.kind) {
    case Ex::SET: return 1;
    case Ex::LOOK: return 0;
    case Ex::CAT:
        for (const Ex &k : e.kids) r += min_len(k);
        return r;
    case Ex::ALT:
        r = ~0ull;
        for (const Ex &k : e.kids) r = std::min(r, min_len(k));
        return r;
    default: return e.lo * min_len(e.kids[0]);
    }
}
static inline bool has_look(const Ex &e)
{
    if (e.kind == Ex::LOOK) return true;
    for (const Ex &k : e.kids)
        if (has_look(k)) return true;
    return false;
}
static inline std::string print(const Ex &e, bool top = false)
{
    std::string s;
    switch (e.kind) {
    case Ex::SET:
    case Ex::LOOK: return e.text;
    case Ex::CAT:
        for (const Ex &k : e.kids) s += k.kind == Ex::ALT ? "(?:" + print(k) + ")" : print(k);
        return s;
    case Ex::ALT:
        for (size_t i = 0; i < e.kids.size(); i++) s += (i ? "|" : "") + print(e.kids[i]);
        return top ? s : "(" + s + ")";
    default: {
        const Ex &k = e.kids[0];
        s = k.kind == Ex::SET ? print(k) : k.kind == Ex::ALT ? print(k) : "(" + print(k) + ")";
        char q[40];
        if (e.lo == 0 && e.hi == 1) return s + "?";
        if (e.lo == 0 && e.hi == ~0u) return s + "*";
        if (e.lo == 1 && e.hi == ~0u) return s + "+";
        if (e.hi == ~0u) snprintf(q, sizeof q, "{%u,}", e.lo);
        else if (e.hi == e.lo) snprintf(q, sizeof q, "{%u}", e.lo);
        else snprintf(q, sizeof q, "{%u,%u}", e.lo, e.hi);
        return s + q;
    }
    }
}

#endif // BZH_REGEX_EX_HOST_H
