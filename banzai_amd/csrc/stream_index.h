// stream_index.h -- the host arithmetic of an index that is written while its stream is: how the entries and sync points of one
// streaming pass, which encodes at bit `phase` of a buffer of its own and counts its blocks and bytes from 0, become entries
// and points of the STREAM (bzs_base, bzs_rebase), how the pending ones are handed out (bzs_take), and the index files of the C
// ABI (bzh_index_blob_*: the blobs BlockIndex.to_bytes() and SyncIndex.to_bytes() write, byte for byte).  No HIP types, no
// context: api.hip calls these, and tests/decode_host/stream_index_host.cpp compiles the same text with g++
// -fsanitize=address,undefined and holds it against a restatement.  An off-by-one here is an index that sends a reader to the
// wrong bit of a 50 GB file.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/bzhip.h"

static_assert(sizeof(bzh_index_entry) == 40 && sizeof(bzh_sync_point) == 288, "the blobs hold these structs as they lie in memory");

// ---- a pass's coordinates -> the stream's --------------------------------------------------------------------------------

struct BzsBase {
    uint64_t bit_add;   // added to every bit position of the pass
    uint64_t out_add;   // added to every out_off
    uint32_t entry_add; // added to every point's entry
};

// A pass starts when `stream_bits` bits of the stream exist (handed out, or carried in the partial word that seeds the pass),
// `consumed` input bytes are encoded and `entries_before` blocks written.  It packs from bit stream_bits % 32 of its own buffer
// (the carried bits lie in front of them in that word), so its bit 0 is the stream's bit stream_bits - stream_bits % 32.
static inline BzsBase bzs_base(uint64_t stream_bits, uint64_t consumed, uint64_t entries_before)
{
    return {stream_bits - (stream_bits & 31u), consumed, (uint32_t)entries_before};
}

static inline void bzs_rebase(const BzsBase &b, bzh_index_entry *e, size_t n, bzh_sync_point *p, size_t np)
{
    for (size_t k = 0; k < n; k++) {
        e[k].bit_pos += b.bit_add;
        e[k].end_bit += b.bit_add;
        e[k].out_off += b.out_add;
    }
    for (size_t k = 0; k < np; k++) {
        p[k].bit_pos += b.bit_add;
        p[k].entry += b.entry_add;
    }
}

// The pending entries and points go out, in order, all or nothing: -> false (nothing removed) when either array is too small.
// *count / *npts are set either way.
static inline bool bzs_take(std::vector<bzh_index_entry> &ents, std::vector<bzh_sync_point> &pts, bzh_index_entry *idx, size_t max,
                            size_t *count, bzh_sync_point *out_pts, size_t max_pts, size_t *npts)
{
    *count = ents.size();
    *npts = pts.size();
    if (ents.size() > max || pts.size() > max_pts) return false;
    if (!ents.empty()) memcpy(idx, ents.data(), ents.size() * sizeof(bzh_index_entry));
    if (!pts.empty()) memcpy(out_pts, pts.data(), pts.size() * sizeof(bzh_sync_point));
    ents.clear();
    pts.clear();
    return true;
}

// ---- index files ---------------------------------------------------------------------------------------------------------
// Block index (interval 0):  "BZhIDX\r\n" | u32 version 1 | u32 reserved 0 | u64 entries | u64 consumed | entries x 40 bytes
// Sync index (interval > 0): "BZhSYN\r\n" | u32 version 1 | u32 interval | u64 bytes of the block index that follows | u64 points
//                            | u32 CRC-32 | u32 reserved 0 | that block index | points x 288 bytes
// All fields little-endian, the arrays as they lie in memory (little-endian hosts only, as the Python classes are).  The CRC
// is zlib's (polynomial 0xEDB88320 reflected, initial value and final XOR all ones) over the 40 header bytes with the CRC field
// zero and everything behind them.

constexpr size_t BZS_IDX_HEAD = 32, BZS_SYN_HEAD = 40;
static const uint8_t BZS_IDX_MAGIC[8] = {'B', 'Z', 'h', 'I', 'D', 'X', '\r', '\n'};
static const uint8_t BZS_SYN_MAGIC[8] = {'B', 'Z', 'h', 'S', 'Y', 'N', '\r', '\n'};
constexpr uint32_t BZS_BLOB_VERSION = 1;

struct BzsCrcTable {
    uint32_t t[256];
    BzsCrcTable()
    {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((c & 1u) ? 0xEDB88320u : 0u);
            t[i] = c;
        }
    }
};
// zlib.crc32(data, crc): continue `crc` (0 to start) over p[0..n)
static inline uint32_t bzs_crc32(uint32_t crc, const uint8_t *p, size_t n)
{
    static const BzsCrcTable tab;
    uint32_t c = ~crc;
    for (size_t k = 0; k < n; k++) c = tab.t[(c ^ p[k]) & 0xFFu] ^ (c >> 8);
    return ~c;
}

static inline void bzs_put32(uint8_t *p, uint32_t v)
{
    for (int k = 0; k < 4; k++) p[k] = (uint8_t)(v >> (8 * k));
}
static inline void bzs_put64(uint8_t *p, uint64_t v)
{
    for (int k = 0; k < 8; k++) p[k] = (uint8_t)(v >> (8 * k));
}
static inline uint32_t bzs_get32(const uint8_t *p)
{
    uint32_t v = 0;
    for (int k = 0; k < 4; k++) v |= (uint32_t)p[k] << (8 * k);
    return v;
}
static inline uint64_t bzs_get64(const uint8_t *p)
{
    uint64_t v = 0;
    for (int k = 0; k < 8; k++) v |= (uint64_t)p[k] << (8 * k);
    return v;
}

// Bytes of the blob for these counts; 0 where they do not belong together (points without an interval, an interval above 32767)
// or the size does not fit a size_t.
static inline size_t bzs_blob_size(size_t count, size_t npts, uint32_t interval)
{
    if (interval > 32767 || (interval == 0 && npts)) return 0;
    const size_t lim = SIZE_MAX - BZS_IDX_HEAD - BZS_SYN_HEAD;
    if (count > lim / sizeof(bzh_index_entry)) return 0;
    const size_t inner = BZS_IDX_HEAD + count * sizeof(bzh_index_entry);
    if (interval == 0) return inner;
    if (npts > (lim - count * sizeof(bzh_index_entry)) / sizeof(bzh_sync_point)) return 0;
    return BZS_SYN_HEAD + inner + npts * sizeof(bzh_sync_point);
}

// -> BZH_OK, BZH_E_ARG (a null pointer where something is claimed, counts that bzs_blob_size refuses), BZH_E_CAP (*out_len set)
static inline int bzs_blob_write(const bzh_index_entry *idx, size_t count, const bzh_sync_point *pts, size_t npts, uint32_t interval,
                                 uint64_t consumed, uint8_t *out, size_t cap, size_t *out_len)
{
    if (!out_len || (!idx && count) || (!pts && npts) || (!out && cap)) return BZH_E_ARG;
    const size_t need = bzs_blob_size(count, npts, interval);
    if (need == 0) return BZH_E_ARG;
    *out_len = need;
    if (need > cap) return BZH_E_CAP;
    const size_t inner = BZS_IDX_HEAD + count * sizeof(bzh_index_entry);
    uint8_t *b = out + (interval ? BZS_SYN_HEAD : 0); // the block index
    memcpy(b, BZS_IDX_MAGIC, 8);
    bzs_put32(b + 8, BZS_BLOB_VERSION);
    bzs_put32(b + 12, 0);
    bzs_put64(b + 16, count);
    bzs_put64(b + 24, consumed);
    if (count) memcpy(b + BZS_IDX_HEAD, idx, count * sizeof(bzh_index_entry));
    if (interval == 0) return BZH_OK;
    if (npts) memcpy(b + inner, pts, npts * sizeof(bzh_sync_point));
    memcpy(out, BZS_SYN_MAGIC, 8);
    bzs_put32(out + 8, BZS_BLOB_VERSION);
    bzs_put32(out + 12, interval);
    bzs_put64(out + 16, inner);
    bzs_put64(out + 24, npts);
    bzs_put32(out + 32, 0);
    bzs_put32(out + 36, 0);
    bzs_put32(out + 32, bzs_crc32(0, out, need));
    return BZH_OK;
}

// The header of a block index blob of exactly n bytes -> its entry count, or false.
static inline bool bzs_idx_head(const uint8_t *b, size_t n, uint64_t *count, uint64_t *consumed)
{
    if (n < BZS_IDX_HEAD || memcmp(b, BZS_IDX_MAGIC, 8) != 0) return false;
    if (bzs_get32(b + 8) != BZS_BLOB_VERSION || bzs_get32(b + 12) != 0) return false;
    *count = bzs_get64(b + 16);
    *consumed = bzs_get64(b + 24);
    const size_t room = n - BZS_IDX_HEAD;
    return *count <= room / sizeof(bzh_index_entry) && *count * sizeof(bzh_index_entry) == room;
}

// -> BZH_OK; BZH_E_ARG (a null blob, count, npts, interval or consumed; a null array with room claimed); BZH_E_DATA (not a
// whole, undamaged blob of either kind); BZH_E_CAP (*count and *npts set, the arrays untouched).  A block index blob gives
// *interval = 0 and *npts = 0.
static inline int bzs_blob_read(const uint8_t *blob, size_t n, bzh_index_entry *idx, size_t max, size_t *count, bzh_sync_point *pts,
                                size_t max_pts, size_t *npts, uint32_t *interval, uint64_t *consumed)
{
    if (!blob || !count || !npts || !interval || !consumed || (!idx && max) || (!pts && max_pts)) return BZH_E_ARG;
    *count = 0;
    *npts = 0;
    *interval = 0;
    *consumed = 0;
    const uint8_t *inner = blob;
    size_t inner_n = n;
    uint64_t np = 0;
    uint32_t iv = 0;
    if (n >= BZS_SYN_HEAD && memcmp(blob, BZS_SYN_MAGIC, 8) == 0) {
        if (bzs_get32(blob + 8) != BZS_BLOB_VERSION) return BZH_E_DATA;
        iv = bzs_get32(blob + 12);
        const uint64_t in64 = bzs_get64(blob + 16);
        np = bzs_get64(blob + 24);
        const size_t room = n - BZS_SYN_HEAD;
        if (iv < 1 || iv > 32767 || in64 > room) return BZH_E_DATA;
        const size_t rest = room - (size_t)in64;
        if (np > rest / sizeof(bzh_sync_point) || np * sizeof(bzh_sync_point) != rest) return BZH_E_DATA;
        if (bzs_get32(blob + 36) != 0) return BZH_E_DATA;
        uint8_t head[BZS_SYN_HEAD];
        memcpy(head, blob, BZS_SYN_HEAD);
        bzs_put32(head + 32, 0);
        if (bzs_crc32(bzs_crc32(0, head, BZS_SYN_HEAD), blob + BZS_SYN_HEAD, room) != bzs_get32(blob + 32)) return BZH_E_DATA;
        inner = blob + BZS_SYN_HEAD;
        inner_n = (size_t)in64;
    }
    uint64_t cnt = 0, cons = 0;
    if (!bzs_idx_head(inner, inner_n, &cnt, &cons)) return BZH_E_DATA;
    *count = (size_t)cnt;
    *npts = (size_t)np;
    *interval = iv;
    *consumed = cons;
    if (cnt > max || np > max_pts) return BZH_E_CAP;
    if (cnt) memcpy(idx, inner + BZS_IDX_HEAD, (size_t)cnt * sizeof(bzh_index_entry));
    if (np) memcpy(pts, inner + inner_n, (size_t)np * sizeof(bzh_sync_point));
    return BZH_OK;
}
