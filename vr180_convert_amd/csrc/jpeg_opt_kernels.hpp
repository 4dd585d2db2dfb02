// jpeg_opt_kernels.hpp -- the device code of the optimised Huffman tables (kernels_jpeg_opt.hip): what a workgroup of the two stages
// does that run between the transform and the size stage of an optimising encode -- the symbol histograms of an image's blocks and the
// table of one histogram -- over the batch's Image and buffer set (jpeg_batch.hpp, jpeg_launch.hpp).  The arithmetic is
// jpeg_core.hpp's block_symbols and jpeg_opt_core.hpp's build_table; here are the staging in LDS, the atomics and the wave's minimum.
#pragma once

#include <hip/hip_runtime.h>

#include "jpeg_kernels.hpp"
#include "jpeg_opt_core.hpp"

namespace v1c {
namespace jpeg {

// What an optimising chunk adds to the Batch: which images build tables of their own, and where their histograms and records lie.
struct OptSlot {
    uint32_t tab;      // the image's entry of the chunk's Tables: its own
    uint32_t ntables;  // 2 (one component) or 4
};

struct OptBatch {
    const int32_t* slot_of;  // per image of the chunk: its slot, or -1 for an image with the Annex K tables
    const OptSlot* slots;
    uint32_t nslots;
    Hist* hist;              // per slot, zeroed
    DhtRecord* rec;          // per slot, zeroed
    Tables* tabs;            // the chunk's Tables, to be filled
};

namespace {

constexpr int kHistWords = 2 * 16 + 2 * 256;  // LDS counters of a workgroup: DC luminance, DC chrominance, AC luminance, AC chrominance

// the LDS counter of a symbol
__device__ inline int hist_word(bool dc, int t, int symbol)
{
    return dc ? t * 16 + symbol : 32 + t * 256 + symbol;
}

// A: the symbols of 256 blocks, one block per lane as in the size stage, counted in LDS and added to the image's histograms once per
// workgroup.  A workgroup has at most 256 * 64 symbols: 32-bit LDS counters hold them; the image's counters are 64-bit.
__device__ __forceinline__ void hist_body(const Image& im, const Buffers& buf, uint32_t wg, Hist* hist, uint32_t (&lds)[256 * kBlockWords],
                                          uint32_t (&identity)[256], uint32_t (&cnt)[kHistWords])
{
    const int tid = threadIdx.x;
    const uint32_t b0 = wg * 256u, b = b0 + tid;
    identity[tid] = identity_entry(tid);
    for (int i = tid; i < kHistWords; i += 256)
        cnt[i] = 0;
    stage_blocks(lds, buf.coef + (size_t)im.blk0 * 64, im.g.nblocks, b0, tid);
    __syncthreads();
    if (b < im.g.nblocks) {
        const int pred = dc_prediction(im, buf.coef, b);
        const int t = block_pos(im.g, b).comp ? 1 : 0;
        block_symbols(StagedBlock{(const int16_t*)(lds + tid * kBlockWords)}, pred, identity,
                      [&](bool dc, int symbol) { atomicAdd(&cnt[hist_word(dc, t, symbol)], 1u); });
    }
    __syncthreads();
    for (int i = tid; i < kHistWords; i += 256) {
        const uint32_t n = cnt[i];
        if (!n)
            continue;
        const bool dc = i < 32;
        const int t = dc ? i >> 4 : (i - 32) >> 8, symbol = dc ? i & 15 : (i - 32) & 255;
        atomicAdd((unsigned long long*)&hist->n[hist_of(dc, t)][symbol], (unsigned long long)n);
    }
}

// the 64 lanes of a wave as the builder's lanes (a workgroup of one wave: the barrier orders its LDS and global accesses)
struct Wave64 {
    __device__ int lane() const { return (int)threadIdx.x; }
    __device__ int lanes() const { return 64; }
    __device__ void barrier() const { __syncthreads(); }
    // every lane gets the two smallest of all lanes' keys (the keys of entries are distinct; kNoEntry stands for none): per round one
    // exchange of both words, not two searches one behind the other -- the chain of dependent cross-lane reads is what a step costs
    __device__ void least_two(uint64_t& k1, uint64_t& k2) const
    {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const uint64_t o1 = (uint64_t)__shfl_xor((unsigned long long)k1, d), o2 = (uint64_t)__shfl_xor((unsigned long long)k2, d);
            const uint64_t lo = k1 < o1 ? k1 : o1, hi = k1 < o1 ? o1 : k1, rest = k2 < o2 ? k2 : o2;
            k1 = lo, k2 = hi < rest ? hi : rest;
        }
    }
};

// B: table t of a slot from its histogram, into the image's Tables and its record; one wave
__device__ __forceinline__ void build_body(const OptBatch& o, uint32_t slot, int t, BuildScratch& s)
{
    const OptSlot sl = o.slots[slot];
    if ((uint32_t)t >= sl.ntables)
        return;
    Tables* tab = o.tabs + sl.tab;
    DhtRecord* r = o.rec + slot;
    build_table(o.hist[slot].n[t], (t & 1) ? 256 : 16, s, (t & 1) ? tab->ac[t >> 1] : tab->dc[t >> 1], r->body[t], &r->len[t], Wave64{});
}

}  // namespace

// the chain of an optimising chunk: launch_encode_batch's kernels with A and B between the transform and the size stage
hipError_t launch_encode_batch_opt(const Batch& b, const OptBatch& o, const uint32_t* first_host, hipStream_t st);

}  // namespace jpeg
}  // namespace v1c
