// kernels_jpegdec.hip -- the device JPEG decoder's kernels for one file: unstuffing of the scan (count, place); the rounds of
// self-synchronising Huffman decoding, one lane per subsequence (init, sync); the last pass from the converged entry states into
// coefficients (write); the DC differences gathered by component for their scan (dcgather); dequantisation and inverse DCT into padded
// component planes (idct); chroma upsampling, colour conversion and the store of BGR rows (colour).  What a workgroup of each does is
// written once, in jpegdec_kernels.hpp, for these kernels and for the batch's (kernels_jpegdec_batch.hip); here are the kernels'
// names, their LDS and their launchers.  The exclusive scans between them are the encoder's (kernels_jpeg.hip: launch_scan).
// INTEGRATION.md section 8 has the contract, DESIGN.md section 14 the design.  A code object of its own: work that decodes nothing does
// not load it.
//
// Nothing waits on another workgroup, and every loop is bounded: the symbol loops by the bits of one subsequence, the code-length loop
// by 16, the segment search by 32 halvings.  Rounds are launches; the host reads flags[] between them.  Wrong entry states are part
// of the scheme, so decode_span (jpegdec_core.hpp) reads only inside the zero-padded unstuffed stream whatever the bits say, and the
// last pass writes only blocks below its segment's quota.
#include <hip/hip_runtime.h>

#include "jpegdec_kernels.hpp"

namespace v1c {
namespace jpegdec {

// Each kernel is its stage's body (jpegdec_kernels.hpp) at workgroup blockIdx.x, over the Args it was launched with.  The body takes
// the kernel's own parameter by reference; a copy of it into a local is what sends the Huffman kernels to scratch.

__global__ __launch_bounds__(256) void k_jdec_count(Args a)
{
    count_body(a, blockIdx.x);
}

__global__ __launch_bounds__(256) void k_jdec_place(Args a)
{
    place_body(a, blockIdx.x);
}

__global__ __launch_bounds__(256) void k_jdec_init(Args a)
{
    init_body(a, blockIdx.x);
}

// Round r raises flags[r & 1] and clears flags[(r + 1) & 1], the next round's; the host reads them between the launches.
__global__ __launch_bounds__(256) void k_jdec_sync(Args a, uint32_t r)
{
    __shared__ Table t[8];
    load_tables(t, a.tab, threadIdx.x);
    __syncthreads();
    sync_body(a, blockIdx.x, r, t, &a.flags[r & 1u], &a.flags[(r + 1) & 1u]);
}

__global__ __launch_bounds__(256) void k_jdec_write(Args a, uint32_t r)
{
    __shared__ Table t[8];
    load_tables(t, a.tab, threadIdx.x);
    __syncthreads();
    write_body(a, blockIdx.x, r, t, &a.flags[2]);
}

__global__ __launch_bounds__(256) void k_jdec_dcgather(Args a)
{
    dcgather_body(a, blockIdx.x);
}

__global__ __launch_bounds__(256) void k_jdec_idct(Args a)
{
    __shared__ int tile[32][8][9];
    __shared__ __attribute__((aligned(16))) int16_t zz[32 * 64];
    __shared__ uint16_t q[4][64];
    idct_body(a, blockIdx.x, tile, zz, q);
}

__global__ __launch_bounds__(256) void k_jdec_colour(Args a)
{
    colour_body(a, blockIdx.x);
}

namespace {

dim3 blocks_for(uint64_t n)
{
    return dim3((uint32_t)((n + 255) / 256));
}

}  // namespace

hipError_t launch_unstuff(const Args& a, hipStream_t st)
{
    hipLaunchKernelGGL(k_jdec_count, blocks_for(a.pieces), dim3(256), 0, st, a);
    const hipError_t e = jpeg::launch_scan(a.drop, a.pieces, a.sums, a.dropoff, st);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_jdec_place, blocks_for(a.pieces), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_sync_init(const Args& a, hipStream_t st)
{
    hipLaunchKernelGGL(k_jdec_init, blocks_for(a.nsub), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_sync_round(const Args& a, uint32_t r, hipStream_t st)
{
    hipLaunchKernelGGL(k_jdec_sync, blocks_for(a.nsub), dim3(256), 0, st, a, r);
    return hipGetLastError();
}

hipError_t launch_write(const Args& a, uint32_t r, hipStream_t st)
{
    const hipError_t e = jpeg::launch_scan(a.count, a.nsub, a.sums, a.first, st);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_jdec_write, blocks_for(a.nsub), dim3(256), 0, st, a, r);
    return hipGetLastError();
}

hipError_t launch_pixels(const Args& a, hipStream_t st)
{
    hipLaunchKernelGGL(k_jdec_dcgather, blocks_for(a.g.nblocks), dim3(256), 0, st, a);
    const hipError_t e = jpeg::launch_scan(a.dcd, a.g.nblocks, a.sums, a.dcoff, st);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_jdec_idct, dim3((a.g.nblocks + 31) / 32), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_jdec_colour, blocks_for((uint64_t)((a.g.w + 3) / 4) * a.g.h), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace jpegdec
}  // namespace v1c
