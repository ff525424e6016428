// decode_stream_plan.h -- the chain walk of bzh_dstream_*: decode_chain_run's walk made resumable over a sliding window of the
// input, and the zlib-shaped feed loop around it.  No HIP types: the GPU is behind `Dev`, which holds the window and the staging
// buffer and is the source of a pass's scan hits, of the results (BzdResult) of its candidates and of the sizes and CRCs of the
// blocks the walk selects; decode.hip's DStreamDev is the real one, and tests/decode_host/dstream_host.cpp compiles the same
// text with g++ -fsanitize=address,undefined over a made-up world and holds it against a restatement that walks the whole
// buffer once and knows no windows.
//
// What is carried from pass to pass: the absolute bit of the next expected item (pos), stream, block, level, the running stream
// CRC, the absolute output total, consumed, finished -- and the candidates not yet passed, as absolute positions (they are
// shifted to window coordinates only for upload).
//
// A PASS (window full, or eof) is one batch: scan the appended bytes, entropy-decode the first candidates of the window, walk the
// chain through them, size the chain's blocks, take as many as the staging room holds, expand and check them, release the bytes
// in front of the first item not taken, move the tail to the front.  Differences to the one-shot walk:
//   undecided is not an error until eof   a block that reports BZD_K_TRUNC, an expected position with fewer than 48 bits behind it,
//                                         a footer with fewer than 4 bytes behind its padding (its `follow` -- input ends / next
//                                         stream / foreign bytes -- cannot be trusted yet) end the pass's chain in front of them.
//   any other kind is final at once       the bits in front of the window's end are the bits bzh_decode sees.
//   staging                               the first block that does not fit the staging room, and all behind it, wait; a first
//                                         block larger than the room makes the room grow to that block.
//   the window grows                      when it is full and the first item of the chain is undecided: by what the call still
//                                         holds, up to max(target, BZS_BLOCK_BYTES_MAX); at that size a block still cut is judged
//                                         as with eof (truncated).
// Dev (every int is a status, 0 = fine; window coordinates = bytes / bits from the window's first byte):
//   uint32_t max_batch()
//   int win_reserve(uint64_t cap, uint64_t keep)                     room for cap bytes, the first `keep` survive
//   int win_append(uint64_t at, const uint8_t *src, uint64_t n)
//   int win_move(uint64_t from, uint64_t len)                        [from, from + len) to the front (the ranges may overlap)
//   int scan(uint64_t from, uint64_t to, std::vector<uint64_t> &hits)   magics wholly inside bytes [from, to): (bit << 1 | footer), ascending
//   int entropy(const uint64_t *cands, uint32_t B, uint64_t held, BzdResult *res)
//   int sizes(std::vector<BzsBlock> &blocks, uint32_t Bu, uint32_t nmax_all)     size / bad_end of each
//   int stage_reserve(uint64_t cap)
//   int emit(std::vector<BzsBlock> &blocks, size_t taken)            blocks[0, taken) to staging at their base; crc of each
//   int handout(uint64_t off, uint8_t *out, uint64_t n)
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "decode_core.h"

constexpr int BZS_OK = 0, BZS_E_ARG = -1, BZS_E_STATE = -5, BZS_E_DATA = -6; // (bzh_status values: decode.hip asserts that they are)

// The largest block the parser accepts, from decode_core.h's own limits: magic, CRC, randomised bit, origPtr; the symbol map (16 +
// 16 * 16); table and selector counts; BZD_MAX_SEL selectors of at most 6 bits (bzd_parse_header refuses a seventh); six tables of
// a 5-bit start and 258 delta-coded lengths; BZD_MAX_SEL groups of BZD_GROUP codes of BZD_MAX_LEN bits.  The delta code of a
// length has no bound in the format (it may step up and down for ever); counted is what the longest walk without a turn needs,
// BZD_MAX_LEN - 1 steps of two bits and the stop bit.  A header that wanders beyond that in a window of this size is called
// truncated.  + 2 bytes: the block begins and ends at any bit of a byte.
constexpr uint64_t BZS_BLOCK_BITS_MAX = 48 + 32 + 1 + 24 + (16 + 16 * 16) + (3 + 15) + 6ull * BZD_MAX_SEL +
                                        6ull * (5 + 258ull * (2 * (BZD_MAX_LEN - 1) + 1)) + (uint64_t)BZD_MAX_SEL * BZD_GROUP * BZD_MAX_LEN;
constexpr uint64_t BZS_BLOCK_BYTES_MAX = BZS_BLOCK_BITS_MAX / 8 + 2;
constexpr uint64_t BZS_ROOM_MIN = 1024;

struct BzsStats { // bzh_dstream_stats, field for field, then what only the host test asks for
    uint64_t passes, blocks, streams, blocks_redone, tail_moves, window_grows, staging_grows, in_bytes, out_bytes, window_peak, staging_peak;
    uint64_t footer_waits, straddles, forced;
};
struct BzsError {     // of the failure that closed the stream
    uint32_t kind;    // BzdKind; BZD_OK: a stream of a level above the context's (`level`)
    uint32_t level;
    uint64_t bit;     // absolute
    size_t stream, block;
    const char *what; // may be null
};
struct BzsBlock {      // a block of the pass's chain (decode.hip: a BackBlock)
    uint32_t slot, nblock;
    uint64_t size = 0; // sizes()
    bool bad_end = false;
    uint64_t base = 0; // in staging
    uint32_t crc = 0;  // emit()
};
struct BzsItem { // what the chain met in a pass, in order, with the walk's state behind it
    bool footer;
    uint32_t crc; // stored
    size_t stream, block;
    uint64_t bit; // absolute
    uint64_t pos_after;
    size_t stream_after, block_after;
    uint32_t level_after;
    bool finishes;
    uint64_t end_byte; // footer: first byte behind its padding, absolute
};

template <class Dev>
struct BzsStream {
    Dev *dev = nullptr;
    int ctx_level = 9;
    uint64_t win_target = 0, stage_target = 0;
    // the stream
    bool open = false, done = false;
    int status = BZS_OK;
    BzsError err{};
    BzsStats st{};
    // the walk between passes
    bool header_done = false, finished = false;
    uint64_t pos = 0;
    size_t stream = 0, block = 0;
    uint32_t level = 0, stream_crc = 0;
    uint64_t total_out = 0, consumed = 0;
    // the window: absolute bytes [base, base + held) in a room of wcap bytes
    uint64_t base = 0, held = 0, wcap = 0;
    uint64_t scanned_to = 0;     // absolute: every magic that ends at or before this byte is in `cands` or passed
    std::vector<uint64_t> cands; // (absolute bit << 1 | footer), ascending, none in front of pos once a pass has dropped them
    uint8_t head[4] = {0, 0, 0, 0};
    bool stuck = false; // the last pass found the first item undecided, and nothing has been appended since
    bool force = false; // the window is as large as a block can be: the first item is judged as with eof
    uint64_t redo_from = 0; // blocks at or behind this bit have not been counted as redone
    // staging
    uint64_t scap = 0, s_len = 0, s_off = 0;
    // scratch of a pass
    std::vector<uint64_t> hits, up;
    std::vector<BzdResult> res;
    std::vector<BzsItem> items;
    std::vector<BzsBlock> blocks;

    uint64_t abs_end() const { return base + held; }
    uint64_t win_limit() const { return win_target > BZS_BLOCK_BYTES_MAX ? win_target : BZS_BLOCK_BYTES_MAX; }

    int begin(Dev *d, int level_of_ctx, uint64_t window, uint64_t staging)
    {
        *this = BzsStream();
        dev = d;
        ctx_level = level_of_ctx;
        win_target = wcap = window;
        stage_target = scap = staging;
        const int rc = dev->win_reserve(wcap, 0);
        if (rc) return rc;
        st.window_peak = wcap;
        st.staging_peak = 0; // (the staging buffer is made by the first pass that has a block)
        open = true;
        return BZS_OK;
    }

    int fail(int s, uint32_t kind, uint64_t bit, size_t at_stream, size_t at_block, const char *what, uint32_t lv = 0)
    {
        status = s;
        err = BzsError{kind, lv, bit, at_stream, at_block, what};
        open = false;
        s_len = s_off = 0; // the pass that found it hands out nothing
        return s;
    }

    // bzh_dstream_feed.  The pointers have been checked.
    int feed(const uint8_t *in, uint64_t n, bool eof, uint64_t *in_used, uint8_t *out, uint64_t cap, uint64_t *out_len, bool *is_done)
    {
        *in_used = 0;
        *out_len = 0;
        *is_done = false;
        if (!open) return BZS_E_STATE;
        if (done) {
            *in_used = n;
            *is_done = true;
            return BZS_OK;
        }
        for (;;) {
            if (s_off < s_len && *out_len < cap) {
                const uint64_t k = s_len - s_off < cap - *out_len ? s_len - s_off : cap - *out_len;
                const int rc = dev->handout(s_off, out + *out_len, k);
                if (rc) return rc;
                s_off += k;
                *out_len += k;
                st.out_bytes += k;
            }
            if (s_off < s_len) break; // `out` is full
            if (finished) {
                done = *is_done = true;
                *in_used = n; // (what follows the last stream is ignored)
                break;
            }
            if (*in_used < n && held < wcap) {
                const uint64_t k = n - *in_used < wcap - held ? n - *in_used : wcap - held;
                for (uint64_t a = abs_end(); a < 4 && a - abs_end() < k; a++) head[a] = in[*in_used + (a - abs_end())];
                const int rc = dev->win_append(held, in + *in_used, k);
                if (rc) return rc;
                held += k;
                *in_used += k;
                st.in_bytes += k;
                stuck = false;
            }
            const bool eof_now = eof && *in_used == n;
            if (stuck && !eof_now) { // full, and the first item undecided: more room, or the verdict
                const uint64_t rest = n - *in_used;
                if (rest == 0) break;
                if (wcap < win_limit()) {
                    const uint64_t want = wcap + rest < win_limit() ? wcap + rest : win_limit();
                    const int rc = dev->win_reserve(want, held);
                    if (rc) return rc;
                    wcap = want;
                    st.window_grows++;
                    if (wcap > st.window_peak) st.window_peak = wcap;
                    continue;
                }
                force = true;
                st.forced++;
            }
            if (held < wcap && !eof_now) break; // all of `in` is used, and no pass is due
            const uint64_t pos_was = pos;
            const bool header_was = header_done;
            const int rc = pass(eof_now);
            if (rc) return rc;
            const bool progress = pos != pos_was || header_done != header_was || finished;
            if (!progress) {
                if (eof_now || force) return fail(BZS_E_STATE, BZD_OK, pos, stream, block, "a pass at eof decided nothing (internal error)");
                stuck = true;
            }
            force = false;
        }
        return BZS_OK;
    }

    int data_error(uint32_t kind, uint64_t bit, size_t s, size_t b, const char *what = nullptr) { return fail(BZS_E_DATA, kind, bit, s, b, what); }

    int pass(bool eof)
    {
        st.passes++;
        // the appended bytes, from 6 bytes before them: a magic that straddles two scans is found by the later one, and one that
        // ends with the earlier scan's last byte by the earlier one alone
        if (abs_end() > scanned_to) {
            const uint64_t floor_bit = scanned_to >= 6 ? 8 * scanned_to - 47 : 0;
            uint64_t from = scanned_to >= 6 ? scanned_to - 6 : 0;
            if (from < base) from = base; // (released bytes lie in front of the chain)
            const int rc = dev->scan(from - base, held, hits);
            if (rc) return rc;
            for (uint64_t h : hits) {
                const uint64_t bit = (h >> 1) + 8 * base;
                if (bit < floor_bit) continue;
                if (scanned_to && bit < 8 * scanned_to) st.straddles++;
                cands.push_back(bit << 1 | (h & 1ull));
            }
            scanned_to = abs_end();
        }
        const uint64_t nbits = 8 * abs_end();
        if (!header_done) {
            const uint64_t n = abs_end();
            if (n < 4) {
                if (!eof) return BZS_OK;
                return data_error(n && memcmp(head, "BZh", n < 3 ? (size_t)n : 3) != 0 ? BZD_K_MAGIC : BZD_K_TRUNC, n * 8, 0, 0, "no stream header");
            }
            if (head[0] != 'B' || head[1] != 'Z' || head[2] != 'h' || head[3] < '1' || head[3] > '9')
                return data_error(BZD_K_MAGIC, 0, 0, 0, "no \"BZh1\"..\"BZh9\"");
            level = (uint32_t)(head[3] - '0');
            if ((int)level > ctx_level) return fail(BZS_E_ARG, BZD_OK, 0, 0, 0, nullptr, level);
            header_done = true;
            pos = 32;
        }
        size_t ci = 0;
        while (ci < cands.size() && (cands[ci] >> 1) < pos) ci++;
        cands.erase(cands.begin(), cands.begin() + (ptrdiff_t)ci);
        if (cands.empty() || (cands[0] >> 1) != pos) {
            if (pos + 48 > nbits) {
                if (!eof) return BZS_OK;
                return data_error(BZD_K_TRUNC, pos, stream, block, "neither a block nor a footer");
            }
            return data_error(BZD_K_MAGIC, pos, stream, block, "neither a block nor a footer");
        }
        const uint32_t mb = dev->max_batch();
        const uint32_t B = (uint32_t)(cands.size() < mb ? cands.size() : mb);
        up.resize(B);
        for (uint32_t k = 0; k < B; k++) up[k] = ((cands[k] >> 1) - 8 * base) << 1 | (cands[k] & 1ull);
        res.resize(B);
        {
            const int rc = dev->entropy(up.data(), B, held, res.data());
            if (rc) return rc;
        }
        // the chain through the batch
        items.clear();
        blocks.clear();
        uint64_t p = pos, last_footer = consumed;
        size_t s = stream, b = block;
        uint32_t lv = level;
        bool fin = false;
        auto redone = [&](uint64_t bit) {
            if (bit >= redo_from) {
                st.blocks_redone++;
                redo_from = bit + 1;
            }
        };
        for (uint32_t k = 0; k < B && !fin; k++) {
            const uint64_t cpos = cands[k] >> 1;
            if (cpos < p) continue; // inside a payload
            if (cpos != p) {
                if (p + 48 > nbits && !eof) break;
                consumed = last_footer;
                return data_error(p + 48 > nbits ? BZD_K_TRUNC : BZD_K_MAGIC, p, s, b, "neither a block nor a footer");
            }
            const BzdResult &r = res[k];
            const bool is_footer = (cands[k] & 1ull) != 0;
            if (r.kind != BZD_OK) {
                if (r.kind == BZD_K_TRUNC && !eof && !(force && items.empty())) {
                    if (!is_footer) redone(cpos);
                    break;
                }
                consumed = last_footer;
                return data_error(r.kind, r.errpos + 8 * base, s, b);
            }
            const uint64_t end_bit = r.end_bit + 8 * base;
            BzsItem it{};
            it.footer = is_footer;
            it.crc = r.crc;
            it.stream = s;
            it.block = b;
            it.bit = cpos;
            if (!is_footer) {
                if (r.nblock > 100000u * lv) {
                    consumed = last_footer;
                    return data_error(BZD_K_FORMAT, cpos, s, b, "more bytes than the stream's block size");
                }
                blocks.push_back(BzsBlock{k, r.nblock});
                b++;
                p = end_bit;
            } else {
                it.end_byte = end_bit / 8;
                if (!eof && it.end_byte + 4 > abs_end()) { // input ends / next stream / foreign bytes: not known yet
                    st.footer_waits++;
                    break;
                }
                last_footer = it.end_byte;
                if (r.follow & 0x100u) { // the next stream: its errors are errors
                    s++;
                    b = 0;
                    lv = r.follow & 15u;
                    if ((int)lv > ctx_level) {
                        consumed = last_footer;
                        return fail(BZS_E_ARG, BZD_OK, 0, s, 0, nullptr, lv);
                    }
                    p = end_bit + 32;
                } else {
                    fin = true; // the input ends here, or foreign bytes follow
                }
            }
            it.pos_after = p;
            it.stream_after = s;
            it.block_after = b;
            it.level_after = lv;
            it.finishes = fin;
            items.push_back(it);
        }
        if (items.empty()) return BZS_OK;
        // sizes, and how many of the chain's blocks the staging room takes
        size_t taken = 0;
        uint64_t sum = 0;
        if (!blocks.empty()) {
            const uint32_t Bu = blocks.back().slot + 1;
            uint32_t nmax_all = 1; // (the inverse BWT runs over slots: the clean candidates off the chain among them set its size too)
            for (uint32_t q = 0; q < Bu; q++)
                if (!(cands[q] & 1ull) && res[q].kind == BZD_OK && res[q].nblock > nmax_all) nmax_all = res[q].nblock;
            int rc = dev->sizes(blocks, Bu, nmax_all);
            if (rc) return rc;
            if (blocks[0].size > scap) {
                scap = blocks[0].size;
                st.staging_grows++;
            }
            for (; taken < blocks.size(); taken++) {
                if (sum + blocks[taken].size > scap) break;
                blocks[taken].base = sum;
                sum += blocks[taken].size;
            }
        }
        // the items kept: up to the first block not taken
        size_t kept = 0, bq = 0;
        for (; kept < items.size(); kept++)
            if (!items[kept].footer && bq++ == taken) break;
        for (size_t i = kept; i < items.size(); i++)
            if (!items[i].footer) redone(items[i].bit);
        items.resize(kept);
        bq = 0;
        last_footer = consumed;
        for (const BzsItem &it : items) {
            if (it.footer) {
                last_footer = it.end_byte;
            } else if (blocks[bq++].bad_end) { // libbz2 refuses the block; the state machine says where
                consumed = last_footer;
                return data_error(BZD_K_FORMAT, it.bit, it.stream, it.block, "the block ends in four equal bytes without a count");
            }
        }
        if (taken) {
            int rc = dev->stage_reserve(scap);
            if (rc) return rc;
            if (scap > st.staging_peak) st.staging_peak = scap;
            rc = dev->emit(blocks, taken);
            if (rc) return rc;
        }
        // CRCs in chain order: every block's against its header, every stream's fold against its footer
        uint32_t crc = stream_crc;
        uint64_t nstreams = 0;
        bq = 0;
        last_footer = consumed;
        for (const BzsItem &it : items) {
            if (!it.footer) {
                if (blocks[bq++].crc != it.crc) {
                    consumed = last_footer;
                    return data_error(BZD_K_BLOCK_CRC, it.bit, it.stream, it.block);
                }
                crc = ((crc << 1) | (crc >> 31)) ^ it.crc;
            } else {
                last_footer = it.end_byte;
                if (crc != it.crc) {
                    consumed = last_footer;
                    return data_error(BZD_K_STREAM_CRC, it.bit, it.stream, it.block);
                }
                crc = 0;
                nstreams++;
            }
        }
        // commit, release, move the tail
        const BzsItem &last = items.back();
        pos = last.pos_after;
        stream = last.stream_after;
        block = last.block_after;
        level = last.level_after;
        finished = last.finishes;
        stream_crc = crc;
        consumed = last_footer;
        total_out += sum;
        s_len = sum;
        s_off = 0;
        st.blocks += taken;
        st.streams += nstreams;
        const uint64_t end = abs_end(), nb = finished ? end : pos / 8;
        if (nb > base) {
            if (end > nb) {
                const int rc = dev->win_move(nb - base, end - nb);
                if (rc) return rc;
                st.tail_moves++;
            }
            held = end - nb;
            base = nb;
        }
        if (finished) cands.clear();
        return BZS_OK;
    }
};
