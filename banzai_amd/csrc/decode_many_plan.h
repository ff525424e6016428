// decode_many_plan.h -- the chain walk of bzh_decode_many*: one scan of the whole buffer, one chain per input, batches that take
// the candidates of many inputs together.  No HIP types: the GPU is only the source of the results (R: BzdResult) of a batch's
// candidates and of the sizes and CRCs of the blocks the walk met; decode.hip's decode_many_run drives it, and
// tests/decode_host/many_host.cpp compiles the same text with g++ -fsanitize=address,undefined and holds it against a
// restatement that judges every input alone, with no batches at all.
//
// A call:   start();  while (next_batch(max, &first, &B)) { feed(res of cands[first .. first + B));  <sizes of items' blocks>
//           place(cap);  <CRCs of the placed blocks unless over>  check(!over); }  finish();
// An error ends that input's chain and nothing else: its candidates still to come are skipped like candidates inside a payload.
// The entropy kernel is bounded by the buffer, not by the slice, so a block cut at the end of a slice reads on into the gap and
// the next input: whatever it reports, an end behind the slice's last bit is a truncated input -- and a footer looks for the next
// stream header only inside its slice.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "decode_core.h"

constexpr int BZM_OK = 0, BZM_E_ARG = -1, BZM_E_DATA = -6; // (bzh_status values: decode.hip asserts that they are)

struct BzmInput {
    uint64_t off, len; // the slice
    uint8_t head[4];   // its first min(len, 4) bytes
};
struct BzmError {        // of the first failure of an input
    uint32_t kind;       // BzdKind; BZD_OK: a stream of a level above the context's (`level`)
    uint32_t level;
    uint64_t bit;        // inside the slice
    size_t stream, block;
    const char *what;    // may be null
};
struct BzmState {
    int status = BZM_OK;
    bool off_set = false;
    uint64_t consumed = 0, out_off = 0, out_len = 0;
    uint64_t decoded = 0;    // bytes of its blocks placed so far (a failed input's gap is at most this)
    uint32_t stream_crc = 0; // the fold of the stream being walked
    BzmError err{};
};
struct BzmItem { // what the chains met in a batch, in order
    bool footer;
    bool dead;        // its input failed behind it in this batch: not sized, not placed
    uint32_t slot;    // its batch slot
    uint32_t input;
    uint32_t crc;     // stored
    uint32_t nblock;
    size_t stream, block;
    uint64_t bit;     // inside the slice
    // blocks: filled by the caller between feed and place (size, bad_end) and between place and check (got_crc)
    uint64_t size = 0;
    bool bad_end = false;
    uint32_t got_crc = 0;
    // blocks: place()
    bool placed = false;
    uint64_t base = 0;
};

struct BzmWalk {
    const uint64_t *cands = nullptr; // (bit position << 1 | footer), ascending, of the whole buffer
    size_t nc = 0;
    const BzmInput *in = nullptr;
    size_t count = 0;
    int ctx_level = 9;
    std::vector<BzmState> st;
    std::vector<BzmItem> items; // of the batch
    uint64_t off_chain = 0, streams = 0, blocks = 0, failed = 0, total_out = 0;
    bool over = false;
    // the open chain
    size_t ci = 0, k = 0; // next candidate; the input whose chain is open (count: none)
    uint64_t pos = 0;     // the bit it expects next, in the buffer
    size_t stream = 0, block = 0;
    uint32_t level = 0;
    size_t first = 0;     // of the batch
    size_t cursor = 0;    // inputs below it have their out_off

    uint64_t lo_bit(size_t j) const { return 8 * in[j].off; }
    uint64_t hi_bit(size_t j) const { return 8 * (in[j].off + in[j].len); }

    void fail(size_t j, int status, uint32_t kind, uint64_t bit, size_t s, size_t b, const char *what, uint32_t lv = 0)
    {
        if (st[j].status != BZM_OK) return; // (the first failure stands)
        st[j].status = status;
        st[j].err = BzmError{kind, lv, bit, s, b, what};
        failed++;
        for (BzmItem &it : items)
            if (it.input == j && !it.placed) it.dead = true;
        if (j == k) open_from(j + 1);
    }
    void fail_here(uint32_t kind, uint64_t bit_in_buffer, const char *what = nullptr)
    {
        const size_t j = k;
        fail(j, BZM_E_DATA, kind, bit_in_buffer >= lo_bit(j) ? bit_in_buffer - lo_bit(j) : 0, stream, block, what);
    }
    // the chain of the first input from j on whose stream header stands
    void open_from(size_t j)
    {
        for (k = j; k < count; k++) {
            const BzmInput &s = in[k];
            stream = block = 0;
            pos = lo_bit(k) + 32;
            const size_t was = k;
            if (s.len < 4) {
                const bool other = s.len && memcmp(s.head, "BZh", s.len < 3 ? (size_t)s.len : 3) != 0;
                k = count; // (fail() must not open a chain itself)
                fail(was, BZM_E_DATA, other ? BZD_K_MAGIC : BZD_K_TRUNC, s.len * 8, 0, 0, "no stream header");
            } else if (s.head[0] != 'B' || s.head[1] != 'Z' || s.head[2] != 'h' || s.head[3] < '1' || s.head[3] > '9') {
                k = count;
                fail(was, BZM_E_DATA, BZD_K_MAGIC, 0, 0, 0, "no \"BZh1\"..\"BZh9\"");
            } else if ((int)(s.head[3] - '0') > ctx_level) {
                k = count;
                fail(was, BZM_E_ARG, BZD_OK, 0, 0, 0, nullptr, (uint32_t)(s.head[3] - '0'));
            } else {
                level = (uint32_t)(s.head[3] - '0');
                return;
            }
            k = was;
        }
    }
    void start()
    {
        st.assign(count, BzmState{});
        items.clear();
        off_chain = streams = blocks = failed = total_out = 0;
        over = false;
        ci = cursor = 0;
        open_from(0);
    }
    // true: the candidate at the chain's bit exists and lies inside the slice
    bool on_chain(uint64_t c) const { return (c >> 1) == pos && pos + 48 <= hi_bit(k); }
    void no_candidate() { fail_here(pos + 48 > hi_bit(k) ? BZD_K_TRUNC : BZD_K_MAGIC, pos, "neither a block nor a footer"); }

    // The next batch: candidates [*first_out, *first_out + *B), the first of them on the open chain.  False: every chain is closed.
    bool next_batch(uint32_t max, size_t *first_out, uint32_t *B)
    {
        items.clear();
        while (k < count) {
            while (ci < nc && (cands[ci] >> 1) < pos) {
                off_chain++;
                ci++;
            }
            if (ci < nc && on_chain(cands[ci])) break;
            no_candidate(); // (opens the next chain)
        }
        if (k == count) {
            off_chain += nc - ci; // (magics in gaps, in foreign bytes and in inputs that failed)
            ci = nc;
            return false;
        }
        first = *first_out = ci;
        *B = (uint32_t)(nc - ci < max ? nc - ci : max);
        ci += *B;
        return true;
    }

    // The chains through the batch.  res[s]: what the entropy stage made of candidate first + s.
    template <class R>
    void feed(const R *res)
    {
        const uint32_t B = (uint32_t)(ci - first);
        for (uint32_t s = 0; s < B; s++) {
            const uint64_t c = cands[first + s], cpos = c >> 1;
            while (k < count && cpos > pos) no_candidate(); // the chain's bit has no candidate: on with the next chain
            if (k == count || cpos < pos) {
                off_chain++;
                continue;
            }
            if (!on_chain(c)) { // (its magic runs past the slice)
                no_candidate();
                off_chain++;
                continue;
            }
            const R &r = res[s];
            if (r.kind != BZD_OK) {
                fail_here(r.kind, r.errpos);
                continue;
            }
            if (r.end_bit > hi_bit(k)) { // it read on behind the slice: whatever it found there
                fail_here(BZD_K_TRUNC, hi_bit(k));
                continue;
            }
            BzmItem it{};
            it.footer = (c & 1ull) != 0;
            it.slot = s;
            it.input = (uint32_t)k;
            it.crc = r.crc;
            it.nblock = r.nblock;
            it.stream = stream;
            it.block = block;
            it.bit = cpos - lo_bit(k);
            if (!it.footer) {
                if (r.nblock > 100000u * level) {
                    fail_here(BZD_K_FORMAT, cpos, "more bytes than the stream's block size");
                    continue;
                }
                items.push_back(it);
                block++;
                blocks++;
                pos = r.end_bit;
                continue;
            }
            items.push_back(it);
            streams++;
            st[k].consumed = r.end_bit / 8 - in[k].off;
            // the next stream's header is looked for inside the slice only (the kernel looked inside the buffer)
            if ((r.follow & 0x100u) && r.end_bit + 32 <= hi_bit(k)) {
                stream++;
                block = 0;
                level = r.follow & 15u;
                pos = r.end_bit + 32;
                if ((int)level > ctx_level) fail(k, BZM_E_ARG, BZD_OK, 0, stream, 0, nullptr, level);
            } else {
                open_from(k + 1); // the input ends here, or foreign bytes follow
            }
        }
    }

    // Where the batch's blocks go.  In: size / bad_end of every block item that is not dead.  A block that ends in four equal
    // bytes without a count fails its input (libbz2 refuses the block); the blocks of an input that has failed are not placed.
    void place(uint64_t cap)
    {
        for (BzmItem &it : items)
            if (!it.footer && !it.dead && it.bad_end)
                fail(it.input, BZM_E_DATA, BZD_K_FORMAT, it.bit, it.stream, it.block, "the block ends in four equal bytes without a count");
        for (BzmItem &it : items) {
            if (it.footer || it.dead || st[it.input].status != BZM_OK) continue;
            offsets_upto(it.input);
            it.placed = true;
            it.base = total_out;
            total_out += it.size;
            st[it.input].out_len += it.size;
            st[it.input].decoded += it.size;
        }
        if (total_out > cap) over = true; // (sizing goes on: the caller learns the total)
    }
    void offsets_upto(size_t j) // inputs up to j start where the output stands now, unless they have started
    {
        for (; cursor <= j && cursor < count; cursor++)
            if (!st[cursor].off_set) {
                st[cursor].off_set = true;
                st[cursor].out_off = total_out;
            }
    }

    // CRCs in chain order: every placed block's against its header, every stream's fold against its footer.  In: got_crc of the
    // placed blocks.  crcs false: a sizing pass, nothing is compared.
    void check(bool crcs)
    {
        if (!crcs) return;
        for (BzmItem &it : items) {
            BzmState &s = st[it.input];
            if (s.status != BZM_OK) continue;
            if (!it.footer) {
                if (it.got_crc != it.crc) {
                    fail(it.input, BZM_E_DATA, BZD_K_BLOCK_CRC, it.bit, it.stream, it.block, nullptr);
                    continue;
                }
                s.stream_crc = ((s.stream_crc << 1) | (s.stream_crc >> 31)) ^ it.crc;
            } else {
                if (s.stream_crc != it.crc) {
                    fail(it.input, BZM_E_DATA, BZD_K_STREAM_CRC, it.bit, it.stream, it.block, nullptr);
                    continue;
                }
                s.stream_crc = 0;
            }
        }
    }

    void finish()
    {
        items.clear();
        offsets_upto(count ? count - 1 : 0);
        for (BzmState &s : st)
            if (s.status != BZM_OK) s.out_len = 0;
    }
};
