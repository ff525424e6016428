// patset.hip -- a compiled set of patterns on its device (bzh_patset_*): the compile is patset_plan.h's, host-only text; here it is
// uploaded, in one allocation that belongs to no context, and handed to the kernels of search.hip and grep.hip as the matcher of
// patset_core.h.  The entry points that take a set (bzh_search_patset*, bzh_grep_patset*) stand beside their twins in api.hip.
#include "common.h"
#include "patset_core.h"
#include "patset_plan.h"

#include <new>

static_assert(BZM_FOLD_ASCII == BZH_PATSET_FOLD_ASCII && BZM_MAX_PATTERNS == BZH_PATSET_MAX_PATTERNS && BZM_MAX_PATTERN == BZH_SEARCH_MAX_PATTERN,
              "patset_plan.h and bzhip.h name the same bounds");

static int patset_create(bzh_ctx *ctx, const uint8_t *const *pats, const size_t *lens, size_t count, unsigned flags, bzh_patset **out)
{
    BzmPlan plan;
    char why[160];
    if (!bzm_compile(pats, lens, count, flags, plan, why, sizeof why)) {
        bzh_set_error(ctx, "%s", why);
        return BZH_E_ARG;
    }
    // one allocation: cls[256], first[256], pat_no[distinct], table[states * classes] -- every part 4-byte aligned
    const size_t o_first = 256, o_pat = o_first + 512, o_tab = o_pat + plan.pat_no.size() * sizeof(uint32_t);
    const size_t total = (o_tab + (size_t)plan.table_bytes() + 15) & ~(size_t)15;
    std::vector<uint8_t> img(total, 0);
    memcpy(img.data(), plan.cls, 256);
    memcpy(img.data() + o_first, plan.first, 512);
    memcpy(img.data() + o_pat, plan.pat_no.data(), plan.pat_no.size() * sizeof(uint32_t));
    memcpy(img.data() + o_tab, plan.table.data(), (size_t)plan.table_bytes());
    bzh_patset *set = new bzh_patset{};
    set->device = ctx->device;
    set->info = bzh_patset_info{plan.patterns, plan.distinct, plan.min_len, plan.max_len, plan.states, plan.classes, plan.table_bytes()};
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipMalloc((void **)&set->d_mem, total);
    if (e == hipSuccess) e = hipMemcpy(set->d_mem, img.data(), total, hipMemcpyHostToDevice); // (waited for: the image may go)
    if (e != hipSuccess) {
        bzh_set_error(ctx, "pattern set: %zu bytes on device %d -> %s", total, ctx->device, hipGetErrorString(e));
        bzh_patset_destroy(set);
        return e == hipErrorOutOfMemory ? BZH_E_NOMEM : BZH_E_HIP;
    }
    set->d_cls = set->d_mem;
    set->d_first = reinterpret_cast<const uint16_t *>(set->d_mem + o_first);
    set->d_pat_no = reinterpret_cast<const uint32_t *>(set->d_mem + o_pat);
    set->d_table = reinterpret_cast<const uint16_t *>(set->d_mem + o_tab);
    *out = set;
    return BZH_OK;
}

extern "C" int bzh_patset_create(bzh_ctx *ctx, const uint8_t *const *pats, const size_t *lens, size_t count, unsigned flags, bzh_patset **out)
{
    if (!ctx || !out) return BZH_E_ARG;
    *out = nullptr;
    try {
        return patset_create(ctx, pats, lens, count, flags, out);
    } catch (const std::bad_alloc &) {
        bzh_set_error(ctx, "host allocation failed");
        return BZH_E_NOMEM;
    } catch (...) {
        bzh_set_error(ctx, "internal error");
        return BZH_E_STATE;
    }
}

extern "C" void bzh_patset_destroy(bzh_patset *set)
{
    if (!set) return;
    if (set->d_mem) {
        int cur = 0;
        const bool back = hipGetDevice(&cur) == hipSuccess && cur != set->device;
        if (hipSetDevice(set->device) == hipSuccess) (void)hipFree(set->d_mem); // (waits for every kernel that reads it)
        if (back) (void)hipSetDevice(cur);
    }
    delete set;
}

extern "C" int bzh_patset_get_info(const bzh_patset *set, bzh_patset_info *out)
{
    if (!set || !out) return BZH_E_ARG;
    *out = set->info;
    return BZH_OK;
}
