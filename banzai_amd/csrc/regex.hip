// regex.hip -- regular expressions on the device (bzh_regex_*): the compile is regex_plan.h's, host-only text; here its automaton
// is uploaded as patset.hip uploads a trie -- one allocation that belongs to no context -- and becomes a bzh_patset of its own
// kind, which matcher_pick.h hands to the kernels of search.hip and grep.hip as the matcher of regex_core.h.  Every
// window, carry, scan, sink and entry point is the set's.
#include "common.h"
#include "regex_core.h"
#include "regex_plan.h"

#include <new>

static_assert(BZR_FOLD_ASCII == BZH_REGEX_FOLD_ASCII && BZR_DOTALL == BZH_REGEX_DOTALL && BZR_NO_LDS == BZH_REGEX_NO_LDS &&
                  BZR_MAX_SPAN == BZH_REGEX_MAX_SPAN && BZR_MAX_EXPR == BZH_REGEX_MAX_EXPR && BZR_MAX_PATTERNS == BZH_PATSET_MAX_PATTERNS,
              "regex_plan.h and bzhip.h name the same bounds");
static_assert(BZR_MAX_SPAN == BZF_MAX_PATTERN, "a match lies inside the tile's halo and the carry");
static_assert(BZR_LDS_ROWS == BZR_LDS_ENTRIES, "regex_core.h and regex_plan.h name the same bound");
static_assert(sizeof(bzh_regex_info) == 40 && sizeof(bzh_regex_look) == 16, "bzh_regex_info, bzh_regex_look");
static_assert(BZR_SYN_ASSERT == BZH_REGEX_ASSERT && BZR_SYN_WORD == BZH_REGEX_WORD && BZR_SYN_LINE == BZH_REGEX_LINE, "one syntax word");
static_assert(BZR_CTX_EDGE == BZR_LOOK_EDGE && BZR_CTX_NL == BZR_LOOK_NL && BZR_CTX_WORD == BZR_LOOK_WORD && BZR_CTX_OTHER == BZR_LOOK_OTHER,
              "regex_plan.h and regex_core.h number the contexts alike");

static bzh_regex_info regex_info(const BzrPlan &p)
{
    return bzh_regex_info{p.expressions, p.min_len, p.max_len, p.states, p.classes, p.unbounded, p.in_lds, p.table_bytes()};
}

static bzh_regex_look regex_look(const BzrPlan &p) { return bzh_regex_look{p.look_behind, p.look_ahead, p.contexts, 0}; }

static int regex_create(bzh_ctx *ctx, const uint8_t *const *exprs, const size_t *lens, size_t count, unsigned flags, uint32_t max_span, unsigned syntax,
                        bzh_patset **out)
{
    BzrPlan plan;
    char why[200];
    if (!bzr_compile_ex(exprs, lens, count, flags, max_span, syntax, plan, why, sizeof why)) {
        bzh_set_error(ctx, "%s", why);
        return BZH_E_ARG;
    }
    // one allocation: cls[256], first[256 * contexts], pat_no[nterm], table[states * classes], and with assertions pat_ctx[4 nterm],
    // acc_mask[nterm] -- every part 4-byte aligned
    const size_t o_first = 256, o_pat = o_first + 512 * (size_t)plan.contexts, o_tab = o_pat + plan.pat_no.size() * sizeof(uint32_t);
    const size_t o_pctx = (o_tab + (size_t)plan.table_bytes() + 3) & ~(size_t)3, o_mask = o_pctx + plan.pat_ctx.size() * sizeof(uint32_t);
    const size_t total = (o_mask + plan.acc_mask.size() + 15) & ~(size_t)15;
    std::vector<uint8_t> img(total, 0);
    memcpy(img.data(), plan.cls, 256);
    memcpy(img.data() + o_first, plan.first, 512 * (size_t)plan.contexts);
    if (!plan.pat_ctx.empty()) memcpy(img.data() + o_pctx, plan.pat_ctx.data(), plan.pat_ctx.size() * sizeof(uint32_t));
    if (!plan.acc_mask.empty()) memcpy(img.data() + o_mask, plan.acc_mask.data(), plan.acc_mask.size());
    memcpy(img.data() + o_pat, plan.pat_no.data(), plan.pat_no.size() * sizeof(uint32_t));
    memcpy(img.data() + o_tab, plan.table.data(), (size_t)plan.table_bytes());
    bzh_patset *set = new bzh_patset{};
    set->device = ctx->device;
    set->regex = true;
    set->rinfo = regex_info(plan);
    set->nterm = plan.nterm;
    set->look = regex_look(plan);
    for (uint32_t c = 0; c < BZR_CONTEXTS; c++) set->ctx_row |= (uint32_t)plan.ctx_row[c] << (8 * c);
    set->info = bzh_patset_info{plan.expressions, plan.expressions, plan.min_len, plan.max_len, plan.states, plan.classes, plan.table_bytes()};
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipMalloc((void **)&set->d_mem, total);
    if (e == hipSuccess) e = hipMemcpy(set->d_mem, img.data(), total, hipMemcpyHostToDevice); // (waited for: the image may go)
    if (e != hipSuccess) {
        bzh_set_error(ctx, "regex: %zu bytes on device %d -> %s", total, ctx->device, hipGetErrorString(e));
        bzh_patset_destroy(set);
        return e == hipErrorOutOfMemory ? BZH_E_NOMEM : BZH_E_HIP;
    }
    set->d_cls = set->d_mem;
    set->d_first = reinterpret_cast<const uint16_t *>(set->d_mem + o_first);
    set->d_pat_no = reinterpret_cast<const uint32_t *>(set->d_mem + o_pat);
    set->d_table = reinterpret_cast<const uint16_t *>(set->d_mem + o_tab);
    set->d_pat_ctx = reinterpret_cast<const uint32_t *>(set->d_mem + o_pctx);
    set->d_acc_mask = set->d_mem + o_mask;
    *out = set;
    return BZH_OK;
}

extern "C" int bzh_regex_create_ex(bzh_ctx *ctx, const uint8_t *const *exprs, const size_t *lens, size_t count, unsigned flags, uint32_t max_span,
                                   unsigned syntax, bzh_patset **out)
{
    if (!ctx || !out) return BZH_E_ARG;
    *out = nullptr;
    try {
        return regex_create(ctx, exprs, lens, count, flags, max_span, syntax, out);
    } catch (const std::bad_alloc &) {
        bzh_set_error(ctx, "host allocation failed");
        return BZH_E_NOMEM;
    } catch (...) {
        bzh_set_error(ctx, "internal error");
        return BZH_E_STATE;
    }
}

extern "C" int bzh_regex_create(bzh_ctx *ctx, const uint8_t *const *exprs, const size_t *lens, size_t count, unsigned flags, uint32_t max_span,
                                bzh_patset **out)
{
    return bzh_regex_create_ex(ctx, exprs, lens, count, flags, max_span, 0, out);
}

extern "C" int bzh_regex_get_look(const bzh_patset *set, bzh_regex_look *out)
{
    if (!set || !out || !set->regex) return BZH_E_ARG;
    *out = set->look;
    return BZH_OK;
}

extern "C" int bzh_regex_get_info(const bzh_patset *set, bzh_regex_info *out)
{
    if (!set || !out || !set->regex) return BZH_E_ARG;
    *out = set->rinfo;
    return BZH_OK;
}

extern "C" int bzh_regex_check_ex(const uint8_t *const *exprs, const size_t *lens, size_t count, unsigned flags, uint32_t max_span, unsigned syntax,
                                  bzh_regex_info *info, bzh_regex_look *look, char *err, size_t errn)
{
    char why[200] = "";
    try {
        BzrPlan plan;
        if (bzr_compile_ex(exprs, lens, count, flags, max_span, syntax, plan, why, sizeof why)) {
            if (info) *info = regex_info(plan);
            if (look) *look = regex_look(plan);
            if (err && errn) err[0] = 0;
            return BZH_OK;
        }
    } catch (const std::bad_alloc &) {
        snprintf(why, sizeof why, "regex: host allocation failed");
        if (err && errn) snprintf(err, errn, "%s", why);
        return BZH_E_NOMEM;
    } catch (...) {
        snprintf(why, sizeof why, "regex: internal error");
        if (err && errn) snprintf(err, errn, "%s", why);
        return BZH_E_STATE;
    }
    if (err && errn) snprintf(err, errn, "%s", why);
    return BZH_E_ARG;
}

extern "C" int bzh_regex_check(const uint8_t *const *exprs, const size_t *lens, size_t count, unsigned flags, uint32_t max_span, bzh_regex_info *info,
                               char *err, size_t errn)
{
    return bzh_regex_check_ex(exprs, lens, count, flags, max_span, 0, info, nullptr, err, errn);
}
