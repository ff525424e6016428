// unbwt_small.hip -- the inverse BWT of small blocks, one workgroup a block, everything in LDS (bzh_decode_many*).
//
// unbwt_run (bwt.hip) is one global radix pass with look-back tiles over an arena strided for 900,000-byte blocks and then
// log2 n + 2 launches of global gathers: built for a few large blocks.  A block of a few thousand bytes fits in a fraction of
// one CU's LDS, so here ONE launch does the whole transform of every small block of a batch:
//
//   load     the last column L into LDS
//   count    a byte histogram per wavefront over its eighth of the column (LDS atomics)
//   bases    exclusive scan over (byte, wavefront): where each wavefront's bytes of each value go
//   rank     the stable LF^-1 permutation T: T[base[L[i]]++] = i, 64 positions a step by wavefront ballots
//   walk     X[i] = T^i(ptr) by pointer doubling, as unbwt_round does: with X[0..m) and P = T^m known, X[m + i] = P[X[i]] and
//            T^2m = P o P (squared through registers, so one array holds it)
//   emit     S[i] = L[X[i + 1]], i < n, into bt.unbwt_out where unrle_maps expects the block
//
// The rule is unbwt_run's to the letter: the last byte is L[T^n(ptr)], not L[ptr], so a column that is no BWT of anything (a
// cycle of T whose length does not divide n) comes out as libbz2's walk gives it.  tests/unbwt_small_model.py restates these
// phases in NumPy, with the same 16-bit indices, against libbz2's serial walk.
//
// Bounded by construction: every index this kernel follows is an entry of T, a permutation of 0 .. n-1 it built itself from n
// bytes (the scatter positions are the prefix sums of the very counts it took, so they end at n), or ptr, which the entropy
// stage has checked against n (and which is clamped here all the same).  n <= UNBWT_SMALL_MAX is checked before anything.
#include <cstdlib>
#include <cstring>

#include "common.h"

constexpr uint32_t UNBWT_SMALL_MAX = 8192;  // bytes of a block's last column; 16-bit indices would reach 65,536
constexpr uint32_t US_THREADS = 512, US_WAVES = US_THREADS / 64, US_ITEMS = UNBWT_SMALL_MAX / US_THREADS;
static_assert(UNBWT_SMALL_MAX <= 65536 && UNBWT_SMALL_MAX == US_THREADS * 16, "16-bit indices; the load is one uint4 a thread");

// 40,960 bytes: four workgroups share a CU's 160 KiB.  The cursors of the count / rank phases lie where the walk later lies,
// the scratch of the scan where T later lies.  X is stored from X[1] on (X[0] is ptr), so that n entries hold it.
struct UsLds {
    uint8_t L[UNBWT_SMALL_MAX];
    union {
        uint16_t P[UNBWT_SMALL_MAX]; // T, then T^m
        uint32_t scan[US_WAVES + 1];
    };
    union {
        uint16_t X1[UNBWT_SMALL_MAX];   // X1[i] = X[i + 1]
        uint32_t cur[US_WAVES][256];    // cur[w][c]: where wavefront w's next byte c goes
    };
};
static_assert(sizeof(UsLds) == 5 * UNBWT_SMALL_MAX, "LDS budget of the small inverse BWT");

__global__ void __launch_bounds__(US_THREADS) unbwt_small_kernel(const uint8_t *bwt, const uint32_t *nn, const uint32_t *ptrs, uint8_t *out, uint32_t S,
                                                                  const uint32_t *slots)
{
    __shared__ UsLds s;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t b = slots[blockIdx.x], n = nn[b];
    if (n == 0 || n > UNBWT_SMALL_MAX) return; // (the host lists small blocks only)
    const uint32_t ptr = min(ptrs[b], n - 1);
    const uint8_t *Lg = bwt + (size_t)b * S;
    // load: 16 bytes a thread (16-byte aligned, and inside the block's stride: S is a multiple of the sort tile)
    if (tid * 16 < n) *reinterpret_cast<uint4 *>(s.L + tid * 16) = *reinterpret_cast<const uint4 *>(Lg + tid * 16);
    for (uint32_t i = tid; i < US_WAVES * 256; i += US_THREADS) (&s.cur[0][0])[i] = 0;
    __syncthreads();
    // count: wavefront w owns positions [w * seg, (w + 1) * seg), seg a multiple of 64
    const uint32_t seg = (n + 64 * US_WAVES - 1) / (64 * US_WAVES) * 64;
    const uint32_t lo = wave * seg, hi = min(n, lo + seg);
    for (uint32_t i = lo + lane; i < hi; i += 64) atomicAdd(&s.cur[wave][s.L[i]], 1u);
    __syncthreads();
    // bases: thread c sums byte c over the wavefronts; the scan runs over bytes, the wavefronts follow inside a byte
    {
        uint32_t mine = 0;
        if (tid < 256)
            for (uint32_t w = 0; w < US_WAVES; w++) mine += s.cur[w][tid];
        uint32_t total;
        uint32_t at = block_excl_add(mine, s.scan, &total); // (total == n: every position was counted once)
        if (tid < 256)
            for (uint32_t w = 0; w < US_WAVES; w++) {
                const uint32_t c = s.cur[w][tid];
                s.cur[w][tid] = at;
                at += c;
            }
    }
    __syncthreads();
    // rank: 64 positions a step.  same = the lanes of this step that hold my byte; those below me go in front of me.
    for (uint32_t j = lo; j < hi; j += 64) { // (lo, hi: the same in every lane of the wavefront)
        const uint32_t i = j + lane;
        const bool valid = i < hi;
        const uint32_t c = valid ? s.L[i] : 0u;
        uint64_t same = __ballot(valid);
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const bool bit = (c >> k) & 1u;
            const uint64_t has = __ballot(valid && bit);
            same &= bit ? has : ~has;
        }
        if (valid) {
            const uint32_t before = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
            const uint32_t at = s.cur[wave][c];
            s.P[at + before] = (uint16_t)i; // (at + before < n: the cursors are prefix sums of the counts of these same bytes)
            if (before == 0) s.cur[wave][c] = at + (uint32_t)__popcll(same);
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); // the next step reads the cursors this one moved
    }
    __syncthreads();
    // walk: X1[m + r - 1] = X[m + r] = P[X[r]] for r < min(m, n + 1 - m), then P = P o P while another round follows
    for (uint32_t m = 1; m <= n; m <<= 1) {
        const uint32_t ext = min(m, n + 1 - m);
        for (uint32_t r = tid; r < ext; r += US_THREADS) s.X1[m + r - 1] = s.P[r ? (uint32_t)s.X1[r - 1] : ptr];
        if (2 * m > n) break; // X[0 .. n] is complete
        uint16_t sq[US_ITEMS];
#pragma unroll
        for (uint32_t k = 0; k < US_ITEMS; k++) {
            const uint32_t r = tid + k * US_THREADS;
            sq[k] = r < n ? s.P[s.P[r]] : (uint16_t)0;
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < US_ITEMS; k++) {
            const uint32_t r = tid + k * US_THREADS;
            if (r < n) s.P[r] = sq[k];
        }
        __syncthreads();
    }
    __syncthreads();
    // emit: four bytes a thread in one word (the block's slot is word aligned), the ragged end byte by byte
    uint8_t *o = out + (size_t)b * S;
    for (uint32_t q = tid; 4 * q < n; q += US_THREADS) {
        const uint32_t i = 4 * q;
        if (i + 4 <= n) {
            const uint32_t v = (uint32_t)s.L[s.X1[i]] | (uint32_t)s.L[s.X1[i + 1]] << 8 | (uint32_t)s.L[s.X1[i + 2]] << 16 | (uint32_t)s.L[s.X1[i + 3]] << 24;
            *reinterpret_cast<uint32_t *>(o + i) = v;
        } else {
            for (uint32_t k = i; k < n; k++) o[k] = s.L[s.X1[k]];
        }
    }
}

extern "C" size_t bzh_decode_many_small_max(void) { return UNBWT_SMALL_MAX; }

// BZH_UNBWT_SMALL=0 turns the LDS path off: bzh_decode_many* then takes every block through unbwt_run (measurement and tests
// only; read at every call, so that one process can compare the two)
bool unbwt_small_enabled()
{
    const char *e = getenv("BZH_UNBWT_SMALL");
    return !(e && !strcmp(e, "0"));
}

// The inverse BWT of the K batch slots listed at d_slots, each of at most UNBWT_SMALL_MAX bytes: bt.bwt / bt.n / bt.ptr -> bt.unbwt_out
int unbwt_small_run(bzh_ctx *ctx, const uint32_t *d_slots, uint32_t K)
{
    if (K == 0) return BZH_OK;
    const Batch &bt = ctx->bt;
    unbwt_small_kernel<<<dim3(K), US_THREADS, 0, ctx->stream>>>(bt.bwt, bt.n, bt.ptr, bt.unbwt_out, bt.S, d_slots);
    HIP_TRY(ctx, hipGetLastError());
    return BZH_OK;
}

// ---- the first bytes of many slices (the stream headers of bzh_decode_many's inputs), one copy back instead of one an input
__global__ void __launch_bounds__(256) many_heads_kernel(const uint8_t *in, const uint64_t *offs, const uint64_t *lens, uint32_t count, uint32_t *heads)
{
    const uint32_t k = blockIdx.x * 256 + threadIdx.x;
    if (k >= count) return;
    const uint64_t off = offs[k], len = lens[k]; // (the host has checked every slice against the buffer)
    uint32_t v = 0;
    for (uint32_t j = 0; j < 4 && j < len; j++) v |= (uint32_t)in[off + j] << (8 * j);
    heads[k] = v;
}

int many_heads_run(bzh_ctx *ctx, const uint8_t *d_in, const uint64_t *d_offs, const uint64_t *d_lens, uint32_t count, uint32_t *d_heads)
{
    if (count == 0) return BZH_OK;
    many_heads_kernel<<<dim3((count + 255) / 256), 256, 0, ctx->stream>>>(d_in, d_offs, d_lens, count, d_heads);
    HIP_TRY(ctx, hipGetLastError());
    return BZH_OK;
}
