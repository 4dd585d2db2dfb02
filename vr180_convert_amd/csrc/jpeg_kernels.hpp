// jpeg_kernels.hpp -- the device functions the JPEG encoder's two code objects share (kernels_jpeg.hip: one image;
// kernels_jpeg_batch.hip: a batch): the staging of a workgroup's blocks and of the code tables in LDS, the workgroup scan, and the
// bit packer of a block.  In an anonymous namespace, as they were in kernels_jpeg.hip: every code object has its own inlined copy.
#pragma once

#include <hip/hip_runtime.h>

#include "jpeg_launch.hpp"

namespace v1c {
namespace jpeg {

namespace {

constexpr int kBlockWords = 33;  // LDS words per staged block: 32 of coefficients and one of padding (lane i starts on bank i)

// the coefficients of blocks [b0, b0 + 256) of the `nblocks` at `coef` into LDS, read coalesced
__device__ inline void stage_blocks(uint32_t* lds, const int16_t* coef, uint32_t nblocks, uint32_t b0, int tid)
{
    const uint32_t* src = (const uint32_t*)coef + (size_t)b0 * 32;
    const uint32_t nwords = min(256u, nblocks - b0) * 32;
#pragma unroll 4
    for (uint32_t i = tid; i < 256 * 32; i += 256)
        if (i < nwords)
            lds[(i >> 5) * kBlockWords + (i & 31)] = src[i];
}

struct StagedBlock {
    const int16_t* p;
    __device__ int operator()(int k) const { return p[k]; }
};

__device__ inline void load_code_tables(uint32_t (*dc)[16], uint32_t (*ac)[256], const Tables* t, int tid)
{
    if (tid < 32)
        dc[tid >> 4][tid & 15] = t->dc[tid >> 4][tid & 15];
    ac[0][tid] = t->ac[0][tid];
    ac[1][tid] = t->ac[1][tid];
}

// exclusive scan over the 256 lanes of a workgroup; `total` is the sum of all.  wsum: four words of LDS
__device__ inline unsigned long long wg_exclusive_scan(unsigned long long x, unsigned long long* wsum, unsigned long long* total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long incl = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long y = __shfl_up(incl, d);
        incl += lane >= d ? y : 0;
    }
    if (lane == 63)
        wsum[wave] = incl;
    __syncthreads();
    unsigned long long base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const unsigned long long v = wsum[w];
        base += w < wave ? v : 0;
        tot += v;
    }
    __syncthreads();
    *total = tot;
    return base + incl - x;
}

// a block's tokens, most significant bit first, into the zeroed words of `raw` from a given bit on; the bytes lie in stream order
struct Packer {
    uint32_t* w;
    unsigned long long acc = 0;
    int n;  // bits in acc (below 32 between tokens); the first word's leading bits belong to the block in front and stay zero
    bool first = true;
    __device__ Packer(uint32_t* raw, uint64_t bit) : w(raw + (bit >> 5)), n((int)(bit & 31)) {}
    __device__ void operator()(uint32_t bits, int len)
    {
        acc = (acc << len) | bits;
        n += len;
        if (n >= 32) {
            n -= 32;
            const uint32_t word = __builtin_bswap32((uint32_t)(acc >> n));
            acc &= (1ull << n) - 1;
            if (first)
                atomicOr(w, word);  // possibly shared with the blocks in front
            else
                *w = word;
            first = false;
            w++;
        }
    }
    __device__ void finish()
    {
        if (n)
            atomicOr(w, __builtin_bswap32((uint32_t)(acc << (32 - n))));  // possibly shared with the blocks behind
    }
};

}  // namespace

}  // namespace jpeg
}  // namespace v1c
