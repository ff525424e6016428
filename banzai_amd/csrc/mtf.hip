// mtf.hip -- move-to-front + RLE2 (RUNA/RUNB) + symbol histogram for a batch of blocks.
//
// Replaces mtf::mtf_and_rle (reference lib/mtf.rs:14-121).  Same outputs: output: Vec<u16>
// (here syms[b][0..m)), num_syms = names + 2, freqs[258] with freqs[EOB] = 1.
//
// MTF without a list: the position of byte c in the recency list equals the number of present
// symbols whose "key" is larger than c's key, where key = time of last occurrence, and a symbol
// not seen yet has key -1-c (so unseen symbols keep ascending order behind all seen ones --
// the identity initial list of lib/mtf.rs:39-43).  Absent bytes get INT_MIN and never count.
// Keys at a tile entry are a prefix-max over tiles of per-tile last occurrences, so tiles are
// independent: one wavefront walks 2048 bytes with its 256 keys in 4 VGPRs (symbol c lives in
// lane c&63, register c>>6); one step = scalar readlane + 4 ballots/popcounts.  A byte equal to
// the current front symbol (zero run, the common case after a BWT) costs one scalar compare.
//
// RLE2 needs no pass of its own.  A position is non-zero exactly at a run head (a byte that differs from the
// byte before it; position 0 of a block: from name 0, the front of the initial list), so which positions emit
// a symbol, the zero run in front of each, its bijective base-2 digits (lib/mtf.rs:46-65) and every output
// offset follow from the bytes alone: mtf_tile_last counts them per tile, mtf_prefix turns the counts into
// offsets (and writes the trailing run and EOB), and the walk stores the digits and pos+1 of the run heads it
// visits anyway, with the symbol histogram.
#include "common.h"

// (MtfTile, the RLE2 layout of one tile, and run_digits: common.h -- sync_emit.hip reads the layout back)

// ---- dense names ------------------------------------------------------------------------------------
// names[c] = rank of byte c among the present bytes (lib/mtf.rs:17-24).  MTF positions are the same
// over names as over byte values (the renaming keeps order), and text blocks with <= 128 distinct
// bytes then need 2 key registers instead of 4.  Every workgroup rebuilds the table from has_byte.
__device__ __forceinline__ uint32_t build_names(const uint8_t *hasbyte, uint8_t *names /*LDS[256]*/, uint32_t *ls)
{
    // callable by 64..256 threads: thread t handles bytes t, t+blockDim, ...
    const uint32_t per = 256 / blockDim.x, c0 = threadIdx.x * per;
    uint32_t cnt = 0;
    for (uint32_t k = 0; k < per; k++) cnt += hasbyte[c0 + k] ? 1u : 0u;
    uint32_t total;
    uint32_t idx = block_excl_add(cnt, ls, &total);
    for (uint32_t k = 0; k < per; k++) {
        names[c0 + k] = (uint8_t)idx;
        idx += hasbyte[c0 + k] ? 1u : 0u;
    }
    __syncthreads();
    return total;
}

// ---- per-tile last occurrence (indexed by name) and RLE2 layout -------------------------------------
// The layout: a run head is a byte that differs from the byte before it (the walk compares names: the same thing, the
// renaming is one to one on the present bytes).  A run crosses threads, sweeps and tiles, so
// the zero run in front of a head is measured from the last head before it: a max-scan over the threads, carried from
// sweep to sweep; the digits in front of the tile's first head wait for mtf_prefix, which knows the last head of the
// tiles before.
__global__ void __launch_bounds__(256) mtf_tile_last(Batch bt, int32_t *tlast, MtfTile *rt, uint32_t MT, uint32_t TL)
{
    const uint32_t b = blockIdx.y, tile = blockIdx.x;
    const uint32_t n = bt.n[b];
    if (tile * TL >= n) return;
    __shared__ int last[256];
    __shared__ uint8_t names[256];
    __shared__ uint32_t ls[8];
    __shared__ uint32_t lm[2][4]; // per sweep (two sets, in turn: one barrier a sweep) and wavefront: its last run head + 1
    __shared__ int s_first;
    __shared__ uint32_t s_cnt;
    last[threadIdx.x] = -1;
    if (threadIdx.x == 0) {
        s_first = -1;
        s_cnt = 0;
    }
    (void)build_names(bt.hasbyte + (size_t)b * 256, names, ls);
    const uint8_t *s = bt.bwt + (size_t)b * bt.S;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t tcarry = 0; // the tile's last run head in the sweeps before this one, + 1 (0: none)
    uint32_t cnt = 0;    // symbols of my heads
    static_assert(MTF_TILE % 2048 == 0, "256 threads x 8 bytes per sweep");
#pragma unroll 1
    for (uint32_t sub = 0; sub < TL; sub += 2048) {
        const uint32_t p0 = tile * TL + sub + threadIdx.x * 8;
        // (a tile may be shorter than one sweep of the workgroup: 512 bytes in tiny batches)
        const bool live = sub + threadIdx.x * 8 < TL && p0 < n;
        uint32_t hm = 0; // bit k: byte k of my eight is a run head
        uint2 w = make_uint2(0u, 0u);
        if (live) w = *reinterpret_cast<const uint2 *>(s + p0);
        uint32_t pb = wave_from_below(w.y) >> 24; // the byte before my eight (a live thread's lower neighbour is live)
        if (live) {
            const uint64_t w64 = ((uint64_t)w.y << 32) | w.x;
            if (lane == 0 && p0 > 0) pb = s[p0 - 1];
            const uint64_t df = w64 ^ ((w64 << 8) | pb);
#pragma unroll
            for (int k = 0; k < 8; k++)
                if (p0 + k < n && ((uint32_t)(df >> (8 * k)) & 255u)) hm |= 1u << k;
            // position 0 of the block follows the front of the initial list, name 0 (lib/mtf.rs:39-43)
            if (p0 == 0) hm = (hm & ~1u) | (names[w.x & 255u] ? 1u : 0u);
            // only the last byte of a run inside my 8 bytes can be its symbol's last occurrence among them (after a
            // BWT most bytes repeat their neighbour, and equal symbols from one wavefront queue on one LDS word)
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const uint32_t p = p0 + k;
                if (p < n) {
                    const bool more = k < 7 && p + 1 < n && !((hm >> (k + 1)) & 1u);
                    if (!more) atomicMax(&last[names[(uint32_t)(w64 >> (8 * k)) & 255u]], (int)p);
                }
            }
        }
        // the last run head before each thread's bytes (+ 1), then the symbols of its heads
        const uint32_t inc = wave_incl_umax_dpp(hm ? p0 + 32u - (uint32_t)__clz(hm) : 0u);
        uint32_t *lw = lm[(sub >> 11) & 1u];
        if (lane == 63) lw[wave] = inc;
        __syncthreads();
        uint32_t before = max(tcarry, wave_from_below(inc));
        for (int q = 0; q < wave; q++) before = max(before, lw[q]);
        tcarry = max(max(tcarry, max(lw[0], lw[1])), max(lw[2], lw[3]));
        if (hm && before == 0u) s_first = (int)(p0 + (uint32_t)__builtin_ctz(hm)); // (one thread of the tile at most)
        int cur = (int)before - 1;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            if ((hm >> k) & 1u) {
                const int p = (int)(p0 + k);
                cnt += 1u + (cur >= 0 ? run_digits((uint32_t)(p - 1 - cur)) : 0u);
                cur = p;
            }
        }
    }
    cnt = wave_all_add(cnt);
    if (lane == 0 && cnt) atomicAdd(&s_cnt, cnt);
    __syncthreads();
    tlast[((size_t)b * MT + tile) * 256 + threadIdx.x] = last[threadIdx.x];
    if (threadIdx.x == 0) {
        MtfTile t;
        t.first = s_first;
        t.last = (int)tcarry - 1;
        t.cnt = s_cnt;
        t.off = 0;
        rt[(size_t)b * MT + tile] = t;
    }
}

// One workgroup per block: turn per-tile last occurrences into keys at tile entry (exclusive
// running "latest occurrence"), seeded with the initial order; also num_syms.  And the RLE2 layout across the
// tiles: the last run head before every tile, the digits of the run that crosses into it, every tile's output
// offset, the trailing run, EOB and m.  freqs is zeroed here: the walk adds to it.
__global__ void __launch_bounds__(256) mtf_prefix(Batch bt, int32_t *tlast, MtfTile *rt, uint32_t MT, uint32_t TL)
{
    const uint32_t b = blockIdx.x;
    const uint32_t n = bt.n[b];
    const uint32_t ntile = (n + TL - 1) / TL;
    const uint32_t c = threadIdx.x;
    const bool present = bt.hasbyte[(size_t)b * 256 + c] != 0;
    uint32_t cnt = __popcll(__ballot(present));
    __shared__ uint32_t w[4];
    if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = cnt;
    __syncthreads();
    const uint32_t num_names = w[0] + w[1] + w[2] + w[3];
    if (threadIdx.x == 0) bt.nsyms[b] = num_names + 2; // lib/mtf.rs:118
    uint32_t *freqs = bt.freqs + (size_t)b * 258;
    for (uint32_t k = c; k < 258; k += 256) freqs[k] = 0;
    { // the layout, 256 tiles at a time (a block has at most S / 2048 = 440)
        MtfTile *rb = rt + (size_t)b * MT;
        __shared__ int lm[4];
        __shared__ int incl[256];
        __shared__ uint32_t ls[6];
        int carry_in = -1;     // last run head before these 256 tiles
        uint32_t off_base = 0; // symbols before them
        for (uint32_t t0 = 0; t0 < ntile; t0 += 256) {
            const uint32_t t = t0 + c;
            MtfTile me{-1, -1, 0, 0};
            if (t < ntile) me = rb[t];
            incl[c] = max(carry_in, block_incl_max(me.last, lm));
            __syncthreads();
            const int carry = c ? incl[c - 1] : carry_in;
            uint32_t tc = me.cnt;
            if (me.first >= 0) tc += run_digits((uint32_t)(me.first - 1 - carry));
            uint32_t total;
            const uint32_t off = off_base + block_excl_add(tc, ls, &total);
            if (t < ntile) {
                me.last = carry;
                me.off = off;
                rb[t] = me;
            }
            carry_in = incl[255];
            off_base += total;
            __syncthreads();
        }
        if (c == 0) { // the run behind the last head, EOB
            const uint32_t z = (uint32_t)((int)n - 1 - carry_in);
            const uint32_t d = run_digits(z);
            uint16_t *out = bt.syms + (size_t)b * (bt.S + 64);
            uint32_t fa = 0, fb = 0;
            for (uint32_t k = 0; k < d; k++) {
                const uint32_t bit = ((z + 1) >> k) & 1u;
                out[off_base + k] = (uint16_t)bit;
                fa += bit ^ 1u;
                fb += bit;
            }
            const uint32_t eob = num_names + 1; // lib/mtf.rs:30
            out[off_base + d] = (uint16_t)eob;
            bt.m[b] = off_base + d + 1;
            // (freqs were zeroed above by other threads of this workgroup, barriers since)
            atomicAdd(&freqs[0], fa);
            atomicAdd(&freqs[1], fb);
            atomicAdd(&freqs[eob], 1u);
        }
    }
    // thread = name: a never-seen name j sits behind every seen one, in name order (lib/mtf.rs:39-43)
    int run = c < num_names ? -1 - (int)c : INT32_MIN;
    int32_t *t = tlast + (size_t)b * MT * 256 + c;
    uint32_t tile = 0;
    for (; tile + 8 <= ntile; tile += 8) {
        int v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = t[(size_t)(tile + k) * 256];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            t[(size_t)(tile + k) * 256] = run;
            if (v[k] >= 0) run = v[k];
        }
    }
    for (; tile < ntile; tile++) {
        int v = t[(size_t)tile * 256];
        t[(size_t)tile * 256] = run;
        if (v >= 0) run = v;
    }
}

// ---- the walk: one wavefront per tile ---------------------------------------------------------------
__device__ __forceinline__ int rdlane(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
// bit `bit` of v as a sign mask (0 or -1): one bit-field extract.  The empty statement keeps the compiler from seeing through
// it: a ballot of `mask != 0` then compares the mask itself, where the compiler would shift v once more for a sign test.
__device__ __forceinline__ int sign_of_bit(int v, int bit)
{
    int om = __builtin_amdgcn_sbfe(v, bit, 1);
    asm("" : "+v"(om));
    return om;
}

// (the comments `// part: NAME` in the walk are read by scripts/count_valu.py: it counts the compiled vector instructions of
// the code between one such comment and the next, by the compiler's line table)

// ---- the walk, parallel form: 64 run heads at a time ------------------------------------------------------------
// Visiting the changed bytes of a tile one after the other is a scalar chain per byte (with ~160 byte values and
// ~45 % changed bytes it was the second most expensive stage of a step).  Here the lanes of the wavefront
// ARE 64 consecutive run heads (bytes that differ from their predecessor; every other byte has position 0 and leaves
// the list alone).  With E[s] = position of symbol s in the recency list when the chunk begins:
//   * a head whose symbol occurred before in the chunk, last at lane p: its position is the number of distinct symbols
//     between p and itself = the lanes u in (p, l) whose own symbol does not occur in (p, u);
//   * a head whose symbol is new in the chunk: E[c] + the symbols that were behind c in the list and have been seen
//     since the chunk began = the lanes u < l that are first occurrences with E[c_u] > E[c].
//   Both are ONE count over the 64 lanes with per-lane bounds (64 steps of a few vector instructions, no dependent
//   chain); the previous / next occurrence of every lane's symbol come from one match-any (8 ballots).
//   * the list for the next chunk: a seen symbol's position = the distinct symbols whose last occurrence in the chunk
//     is later; an unseen symbol moves back by the seen symbols that were behind it.
// The list at tile entry is the rank of mtf_prefix's keys (lib/mtf.rs:39-43 for the first tile).
// The same 64 lanes emit RLE2: the zero run in front of a head ends at the head before it (the lane below, the last
// head of the 64 before, or the tile's carry from mtf_prefix), its digits and the head's pos+1 go to bt.syms from a
// running offset that starts at the tile's, found by one scan over the lanes' symbol counts.
__global__ void __launch_bounds__(64) mtf_walk_par(Batch bt, const int32_t *tlast, const MtfTile *rt, uint32_t MT, uint32_t TL)
{
    const uint32_t b = blockIdx.y, tile = blockIdx.x;
    const uint32_t n = bt.n[b];
    const uint32_t base_p = tile * TL;
    if (base_p >= n) return;
    const int lane = threadIdx.x;
    __shared__ uint8_t names[256];
    __shared__ uint32_t ls[4];
    __shared__ uint16_t Etab[256];         // list position of every name
    __shared__ __attribute__((aligned(16))) uint32_t MF[8]; // per chunk: the list places of its new symbols, one bit each
    __shared__ uint4 NL[4];                // per chunk and 64 places: the word of MF (x, y), the new symbols above the word (z)
    // (the tile is walked in halves of 1024 bytes so that a wavefront needs under 5 KB of LDS: the walk is a chain of
    // dependent steps per wavefront, what hides its latency is the number of wavefronts a compute unit can hold)
    __shared__ uint8_t hsym[1024];     // names of the run heads of the half, in order
    __shared__ uint16_t hoff[1024];    // their offsets in the half
    __shared__ uint32_t hist[128];     // the tile's heads by position, two 16-bit counters a word (a tile has at most 4,096 heads)
    // (the same in every lane, and said so: what hangs on it -- regs, ebits -- then steers scalar branches, not lane masks)
    const uint32_t num_names = (uint32_t)__builtin_amdgcn_readfirstlane((int)build_names(bt.hasbyte + (size_t)b * 256, names, ls));
    const int32_t *keys = tlast + ((size_t)b * MT + tile) * 256;
    const uint8_t *s = bt.bwt + (size_t)b * bt.S + base_p;
    uint16_t *out = bt.syms + (size_t)b * (bt.S + 64);
    const uint32_t remain = n - base_p;
    const uint32_t tile_len = remain < TL ? remain : TL;
    hist[lane] = 0u;
    hist[64 + lane] = 0u;
    uint32_t woff;    // where the next symbol of the tile goes
    int prevhead;     // the last run head before the 64 in hand (position in the block, -1: none)
    {
        const MtfTile me = rt[(size_t)b * MT + tile];
        woff = (uint32_t)__builtin_amdgcn_readfirstlane((int)me.off);
        prevhead = __builtin_amdgcn_readfirstlane(me.last);
    }
    uint32_t fa = 0, fb = 0; // digits of my lanes' runs, and the RUNB among them
    // ---- list at tile entry: E[name] = names with a larger key
    int k[4] = {keys[lane], keys[64 + lane], keys[128 + lane], keys[192 + lane]};
    int front;
    const uint32_t regs = (num_names + 63u) / 64u; // registers of 64 names in use (text: two or three of four)
    const uint32_t ebits = // bits of a list place
        (uint32_t)__builtin_amdgcn_readfirstlane((int)(num_names > 1u ? 32u - (uint32_t)__clz(num_names - 1u) : 1u));
    {
        uint32_t e[4] = {0, 0, 0, 0};
#pragma unroll
        for (int r = 0; r < 4; r++) {
            if ((uint32_t)r < regs) {
                const int cnt = (int)min(64u, num_names - 64u * r);
                for (int j = 0; j < cnt; j++) {
                    const int kj = rdlane(k[r], j);
#pragma unroll
                    for (int q = 0; q < 4; q++) e[q] += kj > k[q] ? 1u : 0u;
                }
            }
        }
#pragma unroll
        for (int q = 0; q < 4; q++) Etab[q * 64 + lane] = (uint16_t)e[q];
        // the symbol at the head of the list = the byte before the tile (or name 0 at the start of the block)
        int best = k[0], bsym = lane;
#pragma unroll
        for (int q = 1; q < 4; q++)
            if (k[q] > best) {
                best = k[q];
                bsym = q * 64 + lane;
            }
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) {
            const int ob = __shfl_xor(best, d, 64), os = __shfl_xor(bsym, d, 64);
            if (ob > best) {
                best = ob;
                bsym = os;
            }
        }
        front = __builtin_amdgcn_readfirstlane(bsym);
    }
    // ---- half by half: its run heads compacted into LDS (16 bytes a lane), then 64 run heads at a time
    uint32_t carry_last = (uint32_t)front;
    const uint32_t lowlo = (uint32_t)((1ull << lane) - 1ull), lowhi = (uint32_t)(((1ull << lane) - 1ull) >> 32); // the lanes below me
#pragma unroll 1
    for (uint32_t cbase = 0; cbase < tile_len; cbase += 1024) {
        // part: half
        const uint4 raw = *reinterpret_cast<const uint4 *>(s + cbase + lane * 16); // (S is padded: the load stays inside the arena)
        uint32_t in[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const uint32_t w = in[d];
            in[d] = (uint32_t)names[w & 255u] | ((uint32_t)names[(w >> 8) & 255u] << 8) | ((uint32_t)names[(w >> 16) & 255u] << 16) |
                    ((uint32_t)names[w >> 24] << 24);
        }
        const uint32_t clen = tile_len - cbase < 1024 ? tile_len - cbase : 1024;
        uint32_t pw = (uint32_t)__shfl_up((int)in[3], 1, 64);
        if (lane == 0) pw = carry_last << 24;
        uint32_t chg = 0;
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const uint32_t x = in[d];
            const uint32_t df = x ^ ((x << 8) | (pw >> 24));
            chg |= ((df & 0xFFu) ? 1u : 0u) << (4 * d);
            chg |= ((df & 0xFF00u) ? 2u : 0u) << (4 * d);
            chg |= ((df & 0xFF0000u) ? 4u : 0u) << (4 * d);
            chg |= ((df & 0xFF000000u) ? 8u : 0u) << (4 * d);
            pw = x;
        }
        {
            const uint32_t lo = (uint32_t)lane * 16u;
            const uint32_t nv = clen > lo ? (clen - lo < 16u ? clen - lo : 16u) : 0u;
            chg &= (1u << nv) - 1u;
        }
        { // name of the chunk's last byte, for the next half's first comparison
            const uint32_t e = clen - 1;
            const uint32_t w = (uint32_t)rdlane((int)(((e >> 2) & 3u) == 0 ? in[0] : ((e >> 2) & 3u) == 1 ? in[1] : ((e >> 2) & 3u) == 2 ? in[2] : in[3]),
                                                (int)(e >> 4));
            carry_last = (w >> (8 * (e & 3u))) & 255u;
        }
        const uint32_t mine = (uint32_t)__popc(chg);
        const uint32_t inc = wave_incl_add_dpp(mine);
        uint32_t at = inc - mine;
#pragma unroll
        for (int kb = 0; kb < 16; kb++) {
            if (chg & (1u << kb)) {
                hsym[at] = (uint8_t)((in[kb >> 2] >> (8 * (kb & 3))) & 255u);
                hoff[at] = (uint16_t)(lane * 16 + kb);
                at++;
            }
        }
        const uint32_t H = (uint32_t)rdlane((int)inc, 63);
        const bool last_half = cbase + 1024 >= tile_len;
        // 64 run heads at a time (one wavefront: program order is enough between the LDS phases)
#pragma unroll 1
    for (uint32_t hb = 0; hb < H; hb += 64) {
        // part: load+match-any
        const uint32_t idx = hb + (uint32_t)lane;
        // the lanes with a head: the first nact, a mask made on the scalar side
        const uint32_t nact = H - hb < 64u ? H - hb : 64u;
        const unsigned long long am = ~0ull >> (64u - nact);
        const bool act = __builtin_amdgcn_inverse_ballot_w64(am);
        const uint32_t c = act ? hsym[idx] : 0u;
        // (ebits is the same in every chunk; taken afresh here, each test on it is a scalar compare and branch of this chunk,
        // where the compiler otherwise keeps eight lane masks across the loop and negates them with vector instructions)
        uint32_t eb = ebits;
        asm volatile("" : "+s"(eb));
        // lanes with my symbol: match-any over the bits of the name.  Names are dense (build_names), so a name has no bit at
        // or above ebits and a step over such a bit would keep every lane: the steps stop there (uniform).  One sign mask,
        // one ballot and one three-input operation per half of the mask a bit (tile_rank, bwt_msd.h).
        uint32_t mlo = (uint32_t)am, mhi = (uint32_t)(am >> 32);
#pragma unroll
        for (int bit = 0; bit < 8; bit++) {
            if (bit == 0 || (uint32_t)bit < eb) { // (ebits is 1 at least)
                const int om = sign_of_bit((int)c, bit);
                const unsigned long long bm = __builtin_amdgcn_ballot_w64(om != 0);
                mlo = __builtin_amdgcn_bitop3_b32(mlo, (uint32_t)bm, (uint32_t)om, 0x90); // m & ~(bm ^ om)
                mhi = __builtin_amdgcn_bitop3_b32(mhi, (uint32_t)(bm >> 32), (uint32_t)om, 0x90);
            }
        }
        // part: pos+prefix-or+next-list
        // the previous occurrence of my symbol in the chunk: the highest lane of the mask below me (p is read only where
        // there is one)
        const uint32_t blo = mlo & lowlo, bhi = mhi & lowhi;
        const unsigned long long nobelow = __builtin_amdgcn_ballot_w64((blo | bhi) == 0u);
        const unsigned long long firsts = am & nobelow; // new in the chunk: one lane per distinct symbol of the chunk
        const bool isfirst = __builtin_amdgcn_inverse_ballot_w64(firsts);
        const bool isrep = __builtin_amdgcn_inverse_ballot_w64(am & ~nobelow);
        const int p = 63 - __builtin_clzll((((unsigned long long)bhi << 32) | blo) | 1ull);
        const int Eown = (int)Etab[c];
        // A = the lanes below me that are the LAST occurrence of their symbol before me: one lane per distinct symbol
        // seen so far.  They are all lower lanes except the predecessors q_v of the lanes v below me: a prefix OR of
        // one bit per lane by data-parallel primitives on the two halves of the mask, then one lane down: exclusive.
        const unsigned long long xb = (unsigned long long)(isrep ? 1u : 0u) << p;
        const uint32_t ilo = wave_incl_or((uint32_t)xb), ihi = wave_incl_or((uint32_t)(xb >> 32));
        const uint32_t xlo = wave_from_below(ilo), xhi = wave_from_below(ihi);
        // the whole chunk's predecessors (lane 63 of the inclusive scan) are the lanes that are NOT the last of their symbol
        const unsigned long long lasts =
            am & ~(((unsigned long long)(uint32_t)rdlane((int)ihi, 63) << 32) | (uint32_t)rdlane((int)ilo, 63));
        const bool more = hb + 64 < H || !last_half;
        // MF: the places (in the list at chunk entry) of the chunk's new symbols, a bit each -- places are distinct
        if (lane < 8) MF[lane] = 0u;
        if (isfirst) atomicOr(&MF[(uint32_t)Eown >> 5], 1u << ((uint32_t)Eown & 31u));
        // One count over the lanes below me gives the position (v_mbcnt: the bits of a mask below my lane, added to a base):
        //  * a symbol seen before in the chunk, last at lane p: the distinct symbols between p and me = A above lane p;
        //  * a symbol that is new in the chunk: its place in the list at chunk entry + the new symbols BEFORE it in the chunk
        //    that were behind it in the list = the lanes u below me among the chunk's first occurrences whose place E_u is
        //    larger than mine: a comparator over the ballots of the places' bits, most significant first (gt: lanes already
        //    known to be larger, eq: lanes that agree with me so far), on the two halves of the masks with my bit as a sign
        //    mask.  A lane that is no first occurrence starts with eq = 0 and keeps its gt.
        const unsigned long long ab = ~1ull << p;
        uint32_t gtlo = isfirst ? 0u : __builtin_amdgcn_bitop3_b32((uint32_t)ab, xlo, xlo, 0x30); // above p, no predecessor
        uint32_t gthi = isfirst ? 0u : __builtin_amdgcn_bitop3_b32((uint32_t)(ab >> 32), xhi, xhi, 0x30);
        // part: places-comparator
        {
            uint32_t eqlo = isfirst ? (uint32_t)firsts : 0u, eqhi = isfirst ? (uint32_t)(firsts >> 32) : 0u;
#pragma unroll
            for (int bit = 7; bit >= 0; bit--) {
                if ((uint32_t)bit >= eb) continue; // (uniform: places are below the number of names)
                const int om = sign_of_bit(Eown, bit);
                const unsigned long long mb = __builtin_amdgcn_ballot_w64(om != 0) & firsts;
                // In a first occurrence's lane eq stays inside firsts.  If no first occurrence has the bit, or all have it,
                // such a lane's bit agrees with every lane of its eq: nothing moves to gt, nothing leaves eq (uniform skip; on
                // text a chunk's new symbols sit at small places, and the high bits fall out here).
                if (mb == 0ull || mb == firsts) continue;
                uint32_t tlo = __builtin_amdgcn_bitop3_b32(eqlo, (uint32_t)mb, (uint32_t)om, 0x40); // eq & mb & ~om
                uint32_t thi = __builtin_amdgcn_bitop3_b32(eqhi, (uint32_t)(mb >> 32), (uint32_t)om, 0x40);
                asm("" : "+v"(tlo), "+v"(thi), "+v"(eqlo), "+v"(eqhi)); // (these first: eq is then updated in place, no copies)
                gtlo |= tlo;
                gthi |= thi;
                eqlo = __builtin_amdgcn_bitop3_b32(eqlo, (uint32_t)mb, (uint32_t)om, 0x90); // eq & ~(mb ^ om)
                eqhi = __builtin_amdgcn_bitop3_b32(eqhi, (uint32_t)(mb >> 32), (uint32_t)om, 0x90);
            }
        }
        // part: pos+prefix-or+next-list
        const int pos = (int)__builtin_amdgcn_mbcnt_hi(gthi, __builtin_amdgcn_mbcnt_lo(gtlo, isfirst ? (uint32_t)Eown : 0u));
        // part: emit+hist+tail
        { // RLE2: digits of the zero run in front of every head (bijective base 2, lib/mtf.rs:46-65), then pos+1 (lib/mtf.rs:91-92)
            const int g = (int)(base_p + cbase) + (act ? (int)hoff[idx] : 0);
            int pg = (int)wave_from_below((uint32_t)g);
            if (lane == 0) pg = prevhead;
            const uint32_t zz = (uint32_t)(g - pg); // run length + 1
            const uint32_t d = act ? 31u - (uint32_t)__clz(zz) : 0u;
            const uint32_t tot = act ? d + 1u : 0u;
            const uint32_t sc = wave_incl_add_dpp(tot);
            // (a 32-bit byte offset from a scalar base: no 64-bit address arithmetic per store)
            char *ob = reinterpret_cast<char *>(out + woff);
            const uint32_t rel = (sc - tot) << 1;
            for (uint32_t j = 0; j < d; j++) *reinterpret_cast<uint16_t *>(ob + (rel + 2u * j)) = (uint16_t)((zz >> j) & 1u);
            if (act) {
                *reinterpret_cast<uint16_t *>(ob + (rel + 2u * d)) = (uint16_t)(pos + 1);
                atomicAdd(&hist[(uint32_t)pos >> 1], 1u << (16u * ((uint32_t)pos & 1u)));
            }
            fb += (uint32_t)__popc(zz & ((1u << d) - 1u));
            fa += d;
            prevhead = rdlane(g, (int)nact - 1);
            woff += (uint32_t)rdlane((int)sc, 63);
        }
        // part: pos+prefix-or+next-list
        // the list when the next chunk begins: an unseen symbol moves back by the new symbols that were behind it = the
        // bits of MF above its place.  Four lanes lay out a record per 64 places -- the word of MF and the new symbols in the
        // words above it -- and every name reads the record of its place with its own address: a shift and two population
        // counts per name.  (The bit at an unseen name's own place is clear, MF holds new symbols only: no shift by one more;
        // the names the chunk has seen are overwritten below.)
        if (more) {
            uint2 w = make_uint2(0u, 0u);
            if (lane < 4) w = *reinterpret_cast<const uint2 *>(&MF[2 * lane]);
            const uint32_t wc = (uint32_t)__popc(w.x) + (uint32_t)__popc(w.y);
            const uint32_t above = BZH_DPP_SRC(wc, 0x101, 0xF) + BZH_DPP_SRC(wc, 0x102, 0xF) + BZH_DPP_SRC(wc, 0x103, 0xF); // row_shl:1..3
            if (lane < 4) NL[lane] = make_uint4(w.x, w.y, above, 0u);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                if ((uint32_t)q < regs) {
                    const uint32_t e = Etab[q * 64 + lane];
                    const uint4 r = *reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(NL) + ((e >> 2) & 0x30u));
                    Etab[q * 64 + lane] = (uint16_t)(e + r.z + (uint32_t)__popcll((((unsigned long long)r.y << 32) | r.x) >> (e & 63u)));
                }
            }
            // (seen symbols are overwritten: position = distinct symbols whose last occurrence comes later = the last
            // occurrences above my lane: all of them but mine and those below me)
            if (__builtin_amdgcn_inverse_ballot_w64(lasts))
                Etab[c] = (uint16_t)((uint32_t)__popcll(lasts) - 1u -
                                     __builtin_amdgcn_mbcnt_hi((uint32_t)(lasts >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)lasts, 0u)));
        }
    }
    }
    // part: -
    // ---- the tile's histogram: one atomic per non-empty bin
    uint32_t *freqs = bt.freqs + (size_t)b * 258;
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const uint32_t hw = hist[q * 64 + lane], lo = hw & 0xFFFFu, hi = hw >> 16;
        const uint32_t pos0 = 2u * (uint32_t)(q * 64 + lane);
        if (lo) atomicAdd(&freqs[pos0 + 1u], lo);
        if (hi) atomicAdd(&freqs[pos0 + 2u], hi);
    }
    fb = wave_all_add(fb);
    fa = wave_all_add(fa) - fb;
    if (lane == 0) {
        if (fa) atomicAdd(&freqs[0], fa);
        if (fb) atomicAdd(&freqs[1], fb);
    }
}

// MTF + RLE2 for blocks 0..B-1 (bt.bwt / bt.n / bt.hasbyte filled).  tlast and the tiles' layout records
// live in the sort lists, which are free once the BWT is emitted.
int mtf_run(bzh_ctx *ctx, uint32_t B, uint32_t nmax, uint64_t ntotal)
{
    Batch &bt = ctx->bt;
    if (B == 0) return BZH_OK;
    hipStream_t st = ctx->stream;
    // A wavefront walks TL bytes from the recency list at their start, which it first builds from the tile's keys (one step per
    // name: a fifth of the walk of a 2,048-byte tile of text).  Tiles of 4,096 bytes halve that share and still leave a large
    // batch three rounds of wavefronts (100 MB: 8.40 -> 8.34 ms); a small batch needs the wavefronts more (28 MB: 3.39 ->
    // 3.49 ms with 4,096) and keeps 2,048.  8,192: no gain anywhere.
    // (Tiles of 512 bytes for batches of one to four blocks -- more wavefronts for a batch that cannot fill the device -- measured
    // SLOWER: config 2 1.062 -> 1.099 ms, one text block 1.258 -> 1.304 ms: the list a tile's walk starts from costs more than
    // the extra wavefronts return.)
    const uint32_t TL = mtf_tile_bytes(B);
    const uint32_t MT = (bt.S + TL - 1) / TL;
    int32_t *tlast = mtf_tlast(bt);
    MtfTile *rt = mtf_tiles(bt);
    const uint32_t mt = (nmax + TL - 1) / TL;
    {
        KSpan ks(ctx, K_MTF_LAST, ntotal, 2);
        mtf_tile_last<<<dim3(mt, B), 256, 0, st>>>(bt, tlast, rt, MT, TL);
        mtf_prefix<<<dim3(B), 256, 0, st>>>(bt, tlast, rt, MT, TL);
    }
    KSpan ks(ctx, K_MTF_WALK, 3 * ntotal); // the last column in, symbols (<= n, 2 bytes) out
    mtf_walk_par<<<dim3(mt, B), 64, 0, st>>>(bt, tlast, rt, MT, TL);
    HIP_TRY(ctx, hipGetLastError());
    return BZH_OK;
}
