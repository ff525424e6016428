// grep_many_plan.h -- the tables of a grep over many texts in one buffer (bzh_grep_many*, grep_many.hip) and the rooms of such a
// call.  Pure host arithmetic, no launch in it: the library compiles it, and tests/decode_host/grep_many_host.cpp runs it against
// brute force with grep_many_core.h as the device.
//
// THE COST.  A virtual tile is a workgroup's work whatever part of the tile its segment owns: an input shorter than a tile costs a
// tile's work, and a tile that k segments meet is loaded k times.  `shared` counts the tiles of the buffer that stand in the
// table more than once.
#ifndef BZH_GREP_MANY_PLAN_H
#define BZH_GREP_MANY_PLAN_H
#include <vector>

#include "grep_many_core.h"

enum : uint64_t { BZGM_MAX_ROWS = 0x7FFFFFFFull }; // one launch's worth of workgroups

// the segments as a caller names them: text k is bytes [offs[k], offs[k] + lens[k]) of a buffer of n.  They ascend and do not
// overlap, gaps are allowed.  Returns null, or what is wrong with segment *bad
static inline const char *bzgm_check(const uint64_t *offs, const uint64_t *lens, size_t count, uint64_t n, size_t *bad)
{
    uint64_t end = 0;
    for (size_t k = 0; k < count; k++) {
        *bad = k;
        if (offs[k] > n || lens[k] > n - offs[k]) return "past the end of the buffer";
        if (offs[k] < end) return "the segments must ascend and must not overlap";
        end = offs[k] + lens[k];
    }
    return nullptr;
}

struct BzgmPlan {
    std::vector<BzgmSeg> seg;
    std::vector<BzgmRow> row;
    uint64_t rows = 0;   // virtual tiles (counted beyond BZGM_MAX_ROWS too; the table is built only within it)
    uint64_t shared = 0; // tiles of the buffer that more than one segment meets
    uint64_t nonempty = 0;

    // checked segments (bzgm_check).  Returns false where the rows are beyond one launch: no table then
    bool build(const uint64_t *offs, const uint64_t *lens, size_t count)
    {
        seg.assign(count, BzgmSeg{});
        row.clear();
        rows = shared = nonempty = 0;
        uint64_t prev_last = ~0ull, counted = ~0ull; // the last tile of the last non-empty segment; the last tile counted as shared
        for (size_t k = 0; k < count; k++) {
            const uint64_t lo = offs[k], hi = lo + lens[k];
            seg[k].lo = lo, seg[k].hi = hi;
            if (hi == lo) continue;
            const uint64_t t_first = lo / BZF_TILE, t_last = (hi - 1) / BZF_TILE;
            if (t_first == prev_last && counted != t_first) shared++, counted = t_first;
            prev_last = t_last;
            nonempty++;
            seg[k].first = (uint32_t)(rows <= BZGM_MAX_ROWS ? rows : 0);
            seg[k].rows = (uint32_t)(t_last - t_first + 1 <= BZGM_MAX_ROWS ? t_last - t_first + 1 : 0);
            rows += t_last - t_first + 1;
        }
        if (rows > BZGM_MAX_ROWS) return false;
        row.reserve((size_t)rows);
        for (size_t k = 0; k < count; k++)
            for (uint32_t j = 0; j < seg[k].rows; j++) row.push_back(BzgmRow{(uint32_t)k, (uint32_t)(seg[k].lo / BZF_TILE) + j});
        return true;
    }
};

// The rooms of a call: counts are always exact; the gather runs only where every room that is asked for holds the call's totals.
struct BzgmRooms {
    bool want_out = false, want_ent = false;
    uint64_t cap = 0, max = 0;
    bool fits(uint64_t bytes, uint64_t sel) const { return !(want_out && bytes > cap) && !(want_ent && sel > max); }
    bool gather(uint64_t bytes, uint64_t sel) const { return fits(bytes, sel) && (want_out || want_ent) && sel > 0; }
};

#endif // BZH_GREP_MANY_PLAN_H
