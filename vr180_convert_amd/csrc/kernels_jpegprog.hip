// kernels_jpegprog.hip -- the kernels of the device decoder of progressive JPEG files, run once per scan of the file: the rounds of
// self-synchronising decoding, one lane per subsequence (init, sync); the last pass from the converged entry states into the file's
// coefficient store (write); behind a DC first scan the values from the scanned differences (dcput); behind the last scan the DC
// values back to the differences the sequential pixel stage takes (dcsave, dcdiff).  What a lane of each does is jpegprog_core.hpp's,
// which the host harness runs too.  Unstuffing, the exclusive scans, the inverse DCT and the colour stage are the sequential
// decoder's kernels, unchanged.  INTEGRATION.md section 8 has the contract, DESIGN.md section 18 the design.  A code object of its
// own: work that decodes no progressive file does not load it.
//
// Nothing waits on another workgroup, and every loop is bounded: the step loops by the bits of one subsequence (and, in an AC
// refinement scan, by the blocks of an end-of-band run), the code-length loop by 16, the correction loops by 64, the segment search by
// 32 halvings.  Rounds are launches; the host reads flags[] between them.  Wrong entry states are part of the scheme: span() reads
// only inside the zero-padded unstuffed scan and, of the store, only blocks below the scan's count; the last pass writes only blocks
// below its segment's quota.  The store is written with 16-bit stores only: two lanes may write different coefficients of one block.
#include <hip/hip_runtime.h>

#include "jpeg_launch.hpp"
#include "jpegprog_launch.hpp"

namespace v1c {
namespace jpegprog {

namespace {

constexpr int kTableWords = (int)(8 * sizeof(Table) / 4);

// the eight Huffman tables into LDS (Tables: dc[4] and ac[4] lie back to back)
__device__ inline void load_tables(Table* t, const Tables* src, int tid)
{
    const uint32_t* s = (const uint32_t*)&src->dc[0];
    uint32_t* d = (uint32_t*)t;
    for (int i = tid; i < kTableWords; i += 256)
        d[i] = s[i];
}

}  // namespace

// (the lane functions take the kernel's own parameter by reference: a copy of it into a local sends the Huffman kernels to scratch)

__global__ __launch_bounds__(256) void k_jprog_init(ScanArgs a)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < a.nsub)
        init_lane(a, i);
}

// Round r raises flags[r & 1] and clears flags[(r + 1) & 1], the next round's; the host reads them between the launches.
__global__ __launch_bounds__(256) void k_jprog_sync(ScanArgs a, uint32_t r)
{
    __shared__ Table t[8];
    load_tables(t, a.tab, threadIdx.x);
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i == 0)
        a.flags[(r + 1) & 1u] = 0;
    if (i < a.nsub && sync_lane(a, i, r, t))
        a.flags[r & 1u] = 1;
}

__global__ __launch_bounds__(256) void k_jprog_write(ScanArgs a, uint32_t r)
{
    __shared__ Table t[8];
    load_tables(t, a.tab, threadIdx.x);
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.nsub)
        return;
    const uint32_t err = write_lane(a, i, r, t);
    if (err != kNoError)
        atomicMin(&a.flags[2], err);
}

__global__ __launch_bounds__(256) void k_jprog_dcput(ScanArgs a)
{
    const uint32_t u = blockIdx.x * 256u + threadIdx.x;
    if (u < a.sc.nunits)
        dcput_lane(a, u);
}

__global__ __launch_bounds__(256) void k_jprog_dcsave(ScanArgs a)
{
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b < a.g.nblocks)
        dcsave_lane(a, b);
}

__global__ __launch_bounds__(256) void k_jprog_dcdiff(ScanArgs a)
{
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b < a.g.nblocks)
        dcdiff_lane(a, b);
}

namespace {

dim3 blocks_for(uint64_t n)
{
    return dim3((uint32_t)((n + 255) / 256));
}

}  // namespace

hipError_t launch_init(const ScanArgs& a, hipStream_t st)
{
    hipLaunchKernelGGL(k_jprog_init, blocks_for(a.nsub), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_round(const ScanArgs& a, uint32_t r, hipStream_t st)
{
    hipLaunchKernelGGL(k_jprog_sync, blocks_for(a.nsub), dim3(256), 0, st, a, r);
    return hipGetLastError();
}

hipError_t launch_write(const ScanArgs& a, uint32_t r, hipStream_t st)
{
    hipError_t e = jpeg::launch_scan(a.count, a.nsub, a.sums, a.first, st);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_jprog_write, blocks_for(a.nsub), dim3(256), 0, st, a, r);
    if (a.sc.kind == kDCFirst) {
        e = jpeg::launch_scan(a.dd, a.sc.nunits, a.sums, a.ddoff, st);
        if (e != hipSuccess)
            return e;
        hipLaunchKernelGGL(k_jprog_dcput, blocks_for(a.sc.nunits), dim3(256), 0, st, a);
    }
    return hipGetLastError();
}

hipError_t launch_dcdiff(const ScanArgs& a, hipStream_t st)
{
    hipLaunchKernelGGL(k_jprog_dcsave, blocks_for(a.g.nblocks), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_jprog_dcdiff, blocks_for(a.g.nblocks), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace jpegprog
}  // namespace v1c
