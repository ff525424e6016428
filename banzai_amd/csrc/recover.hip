// recover.hip -- the gather of bzh_recover_stream*: the bits of every kept block of a damaged input, each from a source bit of
// its own, laid end to end behind the stream header of the output.  ONE launch for all blocks: a descriptor table (source bit,
// destination bit, bits; the destination bits an ascending prefix sum) goes up once, a thread owns destination words and finds
// the blocks that cover each (recover_gather.h: the per-word rule, shared with the host test).  A wavefront's 64 words are
// 2,048 consecutive destination bits, and a block is more than 80 bits: one binary search per wavefront finds the block its
// first word lies in, and each lane walks on from there, a step or two for real blocks.  The source is read through the
// bounded loader at whatever byte a block's bits start, two overlapping words a lane (neighbouring lanes share them in the
// vector cache); the destination is written in whole words, coalesced.  The one word the body can share with the footer --
// its last, when the body does not end on a word -- is ORed in, as concat_bits (api.hip) does; the caller has zeroed it.
#include "common.h"
#include "recover_gather.h"

constexpr uint32_t RG_THREADS = 256;

// Words [1, wend) of dst: the body.  tail: the body ends inside word wend - 1.
__global__ void __launch_bounds__(RG_THREADS) recover_gather_kernel(uint32_t *dst, uint64_t wend, bool tail, const BzrDesc *d, uint32_t K,
                                                                     const uint8_t *src, uint64_t n)
{
    const uint32_t lane = threadIdx.x & 63u;
    // (the grid starts at word 0, which is the header's and is skipped: a wavefront's 64 words then start on a 256-byte line)
    for (uint64_t word = (uint64_t)blockIdx.x * RG_THREADS + threadIdx.x; word - lane < wend; word += (uint64_t)gridDim.x * RG_THREADS) {
        const uint32_t k0 = bzr_find(d, K, (word - lane) * 32); // (the same search in every lane of the wavefront: one line of the table a step)
        if (word == 0 || word >= wend) continue;
        const uint32_t v = bzr_gather_word(d, K, k0, word, src, n);
        if (tail && word == wend - 1) {
            if (v) atomicOr(dst + word, __builtin_bswap32(v));
        } else {
            dst[word] = __builtin_bswap32(v);
        }
    }
}

// The body of the stream into d_out (4-byte aligned; words [1, ceil((32 + body) / 32)) are written, the last one ORed when the
// body ends inside it: the caller zeroes that one).  descs: dst_bit from 32 on, ascending, summing to body.  No wait.
int recover_gather_run(bzh_ctx *ctx, const uint8_t *d_in, size_t n, const std::vector<BzrDesc> &descs, uint64_t body, uint32_t *d_out)
{
    if (descs.empty() || body == 0) return BZH_OK;
    hipStream_t st = ctx->stream;
    BzrDesc *d_desc = nullptr;
    BZH_TRY(reserve_cut(ctx, ctx->sync_ws, "the sync points", grow_mib, [&](Carver &c) { c.put(d_desc, descs.size()); }));
    HIP_TRY(ctx, hipMemcpyAsync(d_desc, descs.data(), descs.size() * sizeof(BzrDesc), hipMemcpyHostToDevice, st));
    const uint64_t end = 32 + body, wend = (end + 31) / 32;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((wend + RG_THREADS - 1) / RG_THREADS, 16384);
    recover_gather_kernel<<<dim3(grid), RG_THREADS, 0, st>>>(d_out, wend, (end & 31u) != 0, d_desc, (uint32_t)descs.size(), d_in, n);
    HIP_TRY(ctx, hipGetLastError());
    return BZH_OK;
}
