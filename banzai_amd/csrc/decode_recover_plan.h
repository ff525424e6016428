// decode_recover_plan.h -- the walk of bzh_recover*: every block magic of the scan is judged on its own, kept when it verifies and
// reported when it does not; magics inside a kept block are its payload.  No HIP types: the GPU is only the source of the results
// of a batch's candidates and of the sizes and CRCs of the clean ones; decode.hip's decode_recover_run drives it, and
// tests/decode_host/recover_host.cpp compiles the same text with g++ -fsanitize=address,undefined and holds it against a
// restatement that makes one pass over all candidates and knows no batches.
//
// A call:   start();  while (next_batch(max, &first, &B)) { feed(res of cands[first .. first + B));  <size, bad_end, got_crc of items>
//           select();  place(cap);  <expansion of the items kept unless over> }  finish();
// The rules are the ones include/bzhip.h states for bzh_recover.  What carries from batch to batch: the end of the most recent
// kept block (the shadow), the stream headers the walk has accepted, and per entry the run of joined blocks it closes -- a
// block's STREAM_END / STREAM_OK are decided when its footer's result arrives, which may be a batch later.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <map>
#include <vector>

#include "../../include/bzhip.h"
#include "decode_core.h"

struct BzrItem {    // a clean block candidate of the batch, outside the shadow when the batch began: the caller sizes it and folds its CRC
    uint32_t slot;  // its batch slot
    uint32_t nblock;
    // in, between feed and select
    uint64_t size = 0;
    bool bad_end = false;
    uint32_t got_crc = 0;
    // out, select
    bool kept = false;
    uint64_t base = 0; // where its bytes go
};

struct BzrRun {     // per entry: the run of kept JOINED entries that ends in it
    uint32_t level; // of the stream header the run starts behind; 0: it reaches none
    uint32_t fold;  // of the stored CRCs of the run
    bool fits;      // every block of the run is within that level
};

struct BzrWalk {
    const uint64_t *cands = nullptr; // (bit position << 1 | footer), ascending
    size_t nc = 0;
    uint64_t n = 0;     // bytes of the input
    uint8_t head[4] = {0, 0, 0, 0}; // its first min(n, 4) bytes
    int ctx_level = 9;
    std::vector<bzh_recover_entry> entries;
    std::vector<BzrRun> runs; // one per entry
    std::vector<BzrItem> items; // of the batch
    std::vector<BzdResult> res; // of the batch
    std::vector<int32_t> item_of; // per slot: its item, or -1
    std::map<uint64_t, uint32_t> headers; // bit position of every accepted stream header -> its level
    bzh_recover_stats stats{};
    uint64_t shadow_end = 0, total_out = 0;
    bool over = false;
    size_t ci = 0, first = 0;

    void start()
    {
        entries.clear(), runs.clear(), items.clear(), res.clear(), item_of.clear(), headers.clear();
        stats = bzh_recover_stats{};
        shadow_end = total_out = 0;
        over = false;
        ci = first = 0;
        if (n >= 4 && head[0] == 'B' && head[1] == 'Z' && head[2] == 'h' && head[3] >= '1' && head[3] <= '9') headers[0] = (uint32_t)(head[3] - '0');
        for (size_t k = 0; k < nc; k++) stats.candidates += !(cands[k] & 1ull);
    }

    // The next batch: candidates [*first_out, *first_out + *B), the first of them outside the shadow.  False: none is left.
    bool next_batch(uint32_t max, size_t *first_out, uint32_t *B)
    {
        items.clear();
        while (ci < nc && (cands[ci] >> 1) < shadow_end) {
            stats.shadowed++;
            ci++;
        }
        if (ci == nc) return false;
        first = *first_out = ci;
        *B = (uint32_t)(nc - ci < max ? nc - ci : max);
        ci += *B;
        stats.batches++;
        return true;
    }

    // r[s]: what the entropy stage made of candidate first + s.  Fills `items`: the blocks whose size and CRC decide the verdict.
    void feed(const BzdResult *r)
    {
        const uint32_t B = (uint32_t)(ci - first);
        res.assign(r, r + B);
        item_of.assign(B, -1);
        items.clear();
        for (uint32_t s = 0; s < B; s++) {
            const uint64_t c = cands[first + s];
            if ((c & 1ull) || (c >> 1) < shadow_end) continue;
            if (res[s].kind != BZD_OK || res[s].nblock > 100000u * (uint32_t)ctx_level) continue;
            item_of[s] = (int32_t)items.size();
            BzrItem it{};
            it.slot = s;
            it.nblock = res[s].nblock;
            items.push_back(it);
        }
    }

    void on_footer(uint64_t pos, const BzdResult &r)
    {
        stats.footers++;
        const bool intact = r.kind == BZD_OK;
        if (!entries.empty() && entries.back().kind == 0 && entries.back().end_bit == pos) { // the footer of the run that ends here
            bzh_recover_entry &e = entries.back();
            const BzrRun &run = runs.back();
            e.flags |= BZH_REC_STREAM_END;
            if (intact && run.level && run.fits && run.fold == r.crc) {
                e.flags |= BZH_REC_STREAM_OK;
                stats.streams_ok++;
            }
        } else if (intact && r.crc == 0 && pos >= 32 && headers.count(pos - 32)) { // an empty stream: a header, its footer, CRC 0
            stats.streams_ok++;
        }
        if (intact && (r.follow & 0x100u)) headers[r.end_bit] = r.follow & 15u;
    }

    // The verdicts of the batch, in order.  In: size / bad_end / got_crc of every item.
    void select()
    {
        const uint32_t B = (uint32_t)(ci - first);
        const uint64_t nbits = 8 * n;
        for (uint32_t s = 0; s < B; s++) {
            const uint64_t c = cands[first + s], pos = c >> 1;
            if (pos < shadow_end) {
                stats.shadowed++;
                continue;
            }
            const BzdResult &r = res[s];
            if (c & 1ull) {
                on_footer(pos, r);
                continue;
            }
            bzh_recover_entry e{};
            e.bit_pos = pos;
            e.out_off = total_out;
            e.crc = pos + 80 <= nbits ? r.crc : 0;
            BzrItem *it = item_of[s] >= 0 ? &items[(size_t)item_of[s]] : nullptr;
            if (r.kind != BZD_OK) {
                e.kind = r.kind;
                e.err_bit = r.errpos;
            } else if (!it || it->bad_end) { // (no item: more bytes than the context's level holds)
                e.kind = BZD_K_FORMAT;
                e.err_bit = pos;
            } else if (it->got_crc != r.crc) {
                e.kind = BZD_K_BLOCK_CRC;
                e.err_bit = pos;
            }
            BzrRun run{0, 0, false};
            if (e.kind == 0) {
                e.end_bit = r.end_bit;
                e.out_len = (uint32_t)it->size;
                const auto h = pos >= 32 ? headers.find(pos - 32) : headers.end();
                if (h != headers.end()) { // behind a stream header: a run begins
                    e.flags |= BZH_REC_JOINED;
                    run = BzrRun{h->second, r.crc, r.nblock <= 100000u * h->second};
                } else if (!entries.empty() && entries.back().kind == 0 && entries.back().end_bit == pos) {
                    e.flags |= BZH_REC_JOINED;
                    const BzrRun &p = runs.back();
                    run = BzrRun{p.level, ((p.fold << 1) | (p.fold >> 31)) ^ r.crc, p.fits && r.nblock <= 100000u * p.level};
                }
                it->kept = true;
                it->base = total_out;
                total_out += it->size;
                shadow_end = r.end_bit;
                stats.kept++;
            } else {
                stats.lost++;
            }
            entries.push_back(e);
            runs.push_back(run);
        }
    }

    void place(uint64_t cap)
    {
        if (total_out > cap) over = true; // (the walk goes on: the caller learns every entry and the total)
    }

    void finish()
    {
        items.clear();
        stats.out_bytes = total_out;
    }
};

// ---- bzh_recover_stream: the report as a whole, before anything is launched ----------------------------------------------
// The kept entries of an untrusted report against an input of n bytes.  Null: well formed; *body = the bits of the kept blocks,
// *kept their number.  Else what is wrong with entry *bad.
static inline const char *bzr_report_check(const bzh_recover_entry *ent, size_t count, uint64_t n, size_t *bad, uint64_t *body, size_t *kept)
{
    uint64_t prev_end = 0, bits = 0;
    size_t k = 0;
    for (size_t i = 0; i < count; i++) {
        const bzh_recover_entry &e = ent[i];
        *bad = i;
        if (e.kind != 0) {
            if (e.end_bit != 0) return "a lost entry with an end_bit";
            continue;
        }
        if (e.end_bit < e.bit_pos || e.end_bit - e.bit_pos <= 80) return "end_bit is not more than 80 bits behind bit_pos";
        if (e.end_bit / 8 > n || (e.end_bit / 8 == n && (e.end_bit & 7u))) return "end_bit lies behind the input";
        if (e.bit_pos < prev_end) return "the kept entries do not ascend, or overlap";
        prev_end = e.end_bit;
        bits += e.end_bit - e.bit_pos;
        k++;
    }
    *body = bits;
    *kept = k;
    return nullptr;
}
