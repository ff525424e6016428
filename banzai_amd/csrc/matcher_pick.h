// matcher_pick.h -- the one place where a search or a grep picks the matcher its kernels are instantiated with (search.hip,
// grep.hip): the single pattern, a set (patset.hip), or an automaton (regex.hip) with its table in LDS or not, with assertions or
// without -- five matchers (patset_core.h, regex_core.h).
#ifndef BZH_MATCHER_PICK_H
#define BZH_MATCHER_PICK_H
#include "common.h"
#include "regex_core.h"

struct BzfPick { // the window the matcher is for
    uint64_t lim;     // a set's or an automaton's matches end at or in front of it
    uint64_t n;       // the window's text ends here: behind it lies the text's edge
    uint64_t edge_lo; // with assertions: the position no byte lies in front of, ...
    uint32_t ctx_lo;  // ... and the context that stands there
};

// f(the matcher): pat where set is null, else the set or automaton as the kernels take it
template <class F>
static void pick_matcher(const BzfPattern &pat, const bzh_patset *set, uint32_t delim, const BzfPick &w, F &&f)
{
    BzmSet m{};
    if (set) m = BzmSet{set->d_cls, set->d_first, set->d_table, set->d_pat_no, set->info.classes, set->regex ? set->nterm : (uint32_t)set->info.distinct, set->info.max_len, delim, w.lim};
    if (set && set->regex) {
        const BzrAuto a{m, set->info.states * set->info.classes};
        const bool lds = set->rinfo.in_lds != 0;
        if (set->looks()) {
            const BzrLook l{set->d_acc_mask, set->d_pat_ctx, set->look.contexts, set->ctx_row, set->look.look_ahead, w.ctx_lo, w.edge_lo, w.n};
            if (lds) f(BzrMatcher<true, true>{{a, l}, {}});
            else f(BzrMatcher<false, true>{{a, l}, {}});
        } else if (lds) f(BzrMatcher<true, false>{{a}, {}});
        else f(BzrMatcher<false, false>{{a}, {}});
    } else if (set) f(BzmMatcher{m});
    else f(BzfOne{{}, pat});
}

#endif // BZH_MATCHER_PICK_H
