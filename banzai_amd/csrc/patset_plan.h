// patset_plan.h -- a set of byte strings compiled into what the matcher of patset_core.h walks (bzh_patset_create, patset.hip).
// Pure host C++17, no HIP in it: the library compiles it, and tests/decode_host/patset_host.cpp runs it under ASan and UBSan
// against a naive matcher.
//
// THE CLASS MAP.  cls[256] sends a byte to its column of the table.  Bytes that occur in no pattern share the dead class 0, whose
// column is all zeros; only when every byte value occurs is there no dead class, and class 0 is an ordinary one.  With
// BZH_PATSET_FOLD_ASCII the bytes 'A' .. 'Z' get the class of 'a' .. 'z' and the patterns are lowered before they are compiled:
// folding is this map and costs the matcher nothing.  Nothing else folds.
//
// THE TRIE has no failure links (PFAC): the matcher walks it from every start position of the text.  State 0 is the root, and no
// transition leads to it, so an entry 0 means "dead".  Rows are dense: table[state * classes + class], 16-bit entries, `states`
// rows, the root's included -- at most 65,535 states beyond the root.
//
// THE NUMBERING.  Terminal states come first: state t + 1 (t < distinct) ends the t-th distinct pattern in ascending order of
// pattern number, and pat_no[t] is that number -- the lowest index among the patterns that are equal after folding.  So "state <=
// distinct" is the test for a terminal, and the length of the match is the depth of the walk.  The other states follow by depth,
// the shallow rows, which every walk reads, next to each other.
//
// first[256] is the root row behind the class map: first[b] = table[cls[b]], what the matcher keeps in LDS for a walk's first step.
#ifndef BZH_PATSET_PLAN_H
#define BZH_PATSET_PLAN_H
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

enum : uint32_t { BZM_FOLD_ASCII = 1, BZM_MAX_PATTERNS = 65536, BZM_MAX_PATTERN = 256, BZM_MAX_STATES = 65535 };

struct BzmPlan {
    uint64_t patterns = 0, distinct = 0;
    uint32_t min_len = 0, max_len = 0;
    uint32_t states = 0, classes = 0; // rows and columns of the table
    uint8_t cls[256];
    uint16_t first[256];
    std::vector<uint16_t> table;  // [states * classes]
    std::vector<uint32_t> pat_no; // [distinct]
    uint64_t table_bytes() const { return (uint64_t)table.size() * sizeof(uint16_t); }
};

static inline uint8_t bzm_fold(uint8_t b, bool fold) { return fold && b >= 'A' && b <= 'Z' ? (uint8_t)(b + 32) : b; }

// Compiles pats[0 .. count) into `out`.  Returns true, or false with the reason in err[0 .. errn).
static inline bool bzm_compile(const uint8_t *const *pats, const size_t *lens, size_t count, unsigned flags, BzmPlan &out, char *err, size_t errn)
{
    if (count == 0 || count > BZM_MAX_PATTERNS) return snprintf(err, errn, "pattern set: %zu patterns, outside 1..%u", count, (unsigned)BZM_MAX_PATTERNS), false;
    if (!pats || !lens) return snprintf(err, errn, "pattern set: a null array"), false;
    if (flags & ~(unsigned)BZM_FOLD_ASCII) return snprintf(err, errn, "pattern set: flags 0x%x, of which only BZH_PATSET_FOLD_ASCII is defined", flags), false;
    for (size_t i = 0; i < count; i++) {
        if (lens[i] == 0 || lens[i] > BZM_MAX_PATTERN) return snprintf(err, errn, "pattern set: pattern %zu has %zu bytes, outside 1..%u", i, lens[i], (unsigned)BZM_MAX_PATTERN), false;
        if (!pats[i]) return snprintf(err, errn, "pattern set: pattern %zu is null", i), false;
    }
    const bool fold = (flags & BZM_FOLD_ASCII) != 0;

    // the folded patterns end to end, and their order: by bytes, equals by index
    std::vector<size_t> at(count + 1, 0);
    for (size_t i = 0; i < count; i++) at[i + 1] = at[i] + lens[i];
    std::vector<uint8_t> text(at[count]);
    for (size_t i = 0; i < count; i++)
        for (size_t j = 0; j < lens[i]; j++) text[at[i] + j] = bzm_fold(pats[i][j], fold);
    auto cmp3 = [&](uint32_t a, uint32_t b) {
        const size_t la = lens[a], lb = lens[b], m = la < lb ? la : lb;
        const int c = memcmp(text.data() + at[a], text.data() + at[b], m);
        return c ? c : (la < lb ? -1 : la > lb ? 1 : 0);
    };
    std::vector<uint32_t> order(count);
    for (size_t i = 0; i < count; i++) order[i] = (uint32_t)i;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        const int c = cmp3(a, b);
        return c ? c < 0 : a < b;
    });
    std::vector<uint32_t> uniq; // the distinct patterns in byte order, each the lowest index among its equals
    for (size_t i = 0; i < count; i++)
        if (i == 0 || cmp3(order[i - 1], order[i]) != 0) uniq.push_back(order[i]);
    auto lcp = [&](uint32_t a, uint32_t b) {
        const size_t m = lens[a] < lens[b] ? lens[a] : lens[b];
        size_t j = 0;
        while (j < m && text[at[a] + j] == text[at[b] + j]) j++;
        return j;
    };
    uint64_t nodes = 0; // a pattern adds the states behind what it shares with the one before it
    for (size_t i = 0; i < uniq.size(); i++) nodes += lens[uniq[i]] - (i ? lcp(uniq[i - 1], uniq[i]) : 0);
    if (nodes > BZM_MAX_STATES) return snprintf(err, errn, "pattern set: the trie needs %llu states, above %u", (unsigned long long)nodes, (unsigned)BZM_MAX_STATES), false;

    // the trie in depth-first order: node 0 is the root
    struct Node {
        uint32_t parent, depth;
        uint8_t byte;
        int64_t pat; // the pattern that ends here, or -1
    };
    std::vector<Node> node;
    node.reserve((size_t)nodes + 1);
    node.push_back(Node{0, 0, 0, -1});
    std::vector<uint32_t> path(BZM_MAX_PATTERN + 1, 0); // path[d]: the node at depth d of the pattern before
    for (size_t i = 0; i < uniq.size(); i++) {
        const uint32_t p = uniq[i];
        const size_t keep = i ? lcp(uniq[i - 1], p) : 0;
        for (size_t d = keep; d < lens[p]; d++) {
            node.push_back(Node{path[d], (uint32_t)d + 1, text[at[p] + d], -1});
            path[d + 1] = (uint32_t)node.size() - 1;
        }
        node[path[lens[p]]].pat = p;
    }

    // the numbering: terminals by pattern number, then the rest by depth
    std::vector<uint32_t> term, rest;
    for (uint32_t v = 1; v < node.size(); v++) (node[v].pat >= 0 ? term : rest).push_back(v);
    std::sort(term.begin(), term.end(), [&](uint32_t a, uint32_t b) { return node[a].pat < node[b].pat; });
    std::stable_sort(rest.begin(), rest.end(), [&](uint32_t a, uint32_t b) { return node[a].depth < node[b].depth; });
    std::vector<uint16_t> num(node.size(), 0);
    out.pat_no.resize(term.size());
    for (size_t t = 0; t < term.size(); t++) num[term[t]] = (uint16_t)(t + 1), out.pat_no[t] = (uint32_t)node[term[t]].pat;
    for (size_t r = 0; r < rest.size(); r++) num[rest[r]] = (uint16_t)(term.size() + 1 + r);

    // the classes
    bool used[256] = {};
    for (uint8_t b : text) used[b] = true;
    uint32_t nused = 0;
    for (uint32_t b = 0; b < 256; b++) nused += used[b];
    uint32_t next = nused == 256 ? 0 : 1;
    for (uint32_t b = 0; b < 256; b++) out.cls[b] = used[b] ? (uint8_t)next++ : 0;
    if (fold)
        for (uint32_t b = 'A'; b <= 'Z'; b++) out.cls[b] = out.cls[b + 32];
    out.classes = next;
    out.states = (uint32_t)node.size();
    out.table.assign((size_t)out.states * out.classes, 0);
    for (uint32_t v = 1; v < node.size(); v++) out.table[(size_t)num[node[v].parent] * out.classes + out.cls[node[v].byte]] = num[v];
    for (uint32_t b = 0; b < 256; b++) out.first[b] = out.table[out.cls[b]];

    out.patterns = count, out.distinct = uniq.size();
    out.min_len = out.max_len = (uint32_t)lens[0];
    for (size_t i = 1; i < count; i++) out.min_len = std::min<uint32_t>(out.min_len, (uint32_t)lens[i]), out.max_len = std::max<uint32_t>(out.max_len, (uint32_t)lens[i]);
    return true;
}

#endif // BZH_PATSET_PLAN_H
