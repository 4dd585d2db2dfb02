// kernels_jpeg.hip -- the device JPEG encoder's kernels for one image: colour conversion, chroma downsampling, forward DCT and
// quantisation (transform); the coded bits of every block (size); bit packing of the intervals, most significant bit first (pack); the
// 0xFF bytes, and the stuffed intervals with their RSTm markers at their final offsets (count, place); the exclusive scans between
// them.  What a workgroup of each of the six stages does is written once, in jpeg_kernels.hpp, over an Image and a buffer set, for
// these kernels and for the batch's (kernels_jpeg_batch.hip); a kernel here makes the Image whose regions begin at zero and calls the
// body.  The three scan kernels are here and serve the batch and the decoder too.  INTEGRATION.md section 7 has the stream contract,
// DESIGN.md section 13 the design.  A code object of its own: the remap and PNG kernels do not change with it.
//
// The standard Huffman tables are fixed, so the host takes no part between the kernels: they form one chain on the stream.  Every
// lane does a bounded amount of work whatever the restart interval, and nothing waits on another workgroup.  Words of the
// unstuffed stream that two blocks share are written with atomic ORs of disjoint bits into a zeroed buffer, words a block owns
// with plain stores, and every byte of the final stream is written exactly once: the result does not depend on any order.
#include <hip/hip_runtime.h>

#include "jpeg_kernels.hpp"

namespace v1c {
namespace jpeg {

namespace {

// the single call's image: its regions begin where the buffers do
__device__ __forceinline__ Image image_of(const Args& a)
{
    return Image{a.img, a.pitch, a.g, 0, 0, 0, 0, 0};
}

}  // namespace

__global__ __launch_bounds__(256) void k_jpeg_transform(Args a)
{
    __shared__ int tile[32][8][9];
    __shared__ __attribute__((aligned(16))) int16_t zz[32 * 64];
    __shared__ uint16_t q[2][64];
    transform_body(image_of(a), a.tab, a.buf, blockIdx.x, tile, zz, q);
}

__global__ __launch_bounds__(256) void k_jpeg_size(Args a)
{
    __shared__ uint32_t lds[256 * kBlockWords];
    __shared__ uint32_t dc[2][16], ac[2][256];
    size_body(image_of(a), a.tab, a.buf, blockIdx.x, lds, dc, ac);
}

// scans, first step: the sum of every chunk of kScanChunk entries
__global__ __launch_bounds__(256) void k_jpeg_scan_sum(const uint32_t* in, uint64_t n, uint64_t* sums)
{
    __shared__ unsigned long long wsum[4];
    const uint64_t i0 = (uint64_t)blockIdx.x * kScanChunk + threadIdx.x * 8u;
    unsigned long long x = 0;
#pragma unroll
    for (int k = 0; k < 8; k++)
        x += i0 + k < n ? in[i0 + k] : 0u;
    unsigned long long total;
    (void)wg_exclusive_scan(x, wsum, &total);
    if (threadIdx.x == 0)
        sums[blockIdx.x] = total;
}

// scans, second step: the exclusive scan of the chunk sums in place, and the grand total into out[n]; one workgroup
__global__ __launch_bounds__(256) void k_jpeg_scan_top(uint64_t* sums, uint32_t nchunks, uint64_t* out, uint64_t n)
{
    __shared__ unsigned long long wsum[4];
    unsigned long long carry = 0;
    for (uint32_t i0 = 0; i0 < nchunks; i0 += 256) {
        const uint32_t i = i0 + threadIdx.x;
        const unsigned long long v = i < nchunks ? sums[i] : 0;
        unsigned long long total;
        const unsigned long long ex = wg_exclusive_scan(v, wsum, &total);
        if (i < nchunks)
            sums[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0)
        out[n] = carry;
}

// scans, third step: out[i] = the sum of in[0 .. i)
__global__ __launch_bounds__(256) void k_jpeg_scan_apply(const uint32_t* in, uint64_t n, const uint64_t* sums, uint64_t* out)
{
    __shared__ unsigned long long wsum[4];
    const uint64_t i0 = (uint64_t)blockIdx.x * kScanChunk + threadIdx.x * 8u;
    uint32_t v[8];
    unsigned long long x = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        v[k] = i0 + k < n ? in[i0 + k] : 0u;
        x += v[k];
    }
    unsigned long long total;
    unsigned long long at = sums[blockIdx.x] + wg_exclusive_scan(x, wsum, &total);
#pragma unroll
    for (int k = 0; k < 8; k++) {
        if (i0 + k < n)
            out[i0 + k] = at;
        at += v[k];
    }
}

__global__ __launch_bounds__(256) void k_jpeg_interval_bytes(Args a)
{
    interval_bytes_body(image_of(a), a.buf, blockIdx.x);
}

__global__ __launch_bounds__(256) void k_jpeg_pack(Args a)
{
    __shared__ uint32_t lds[256 * kBlockWords];
    __shared__ uint32_t dc[2][16], ac[2][256];
    pack_body(image_of(a), a.tab, a.buf, blockIdx.x, lds, dc, ac);
}

__global__ __launch_bounds__(256) void k_jpeg_count(Args a, uint64_t pieces)
{
    count_body(a.buf, blockIdx.x, pieces);
}

__global__ __launch_bounds__(256) void k_jpeg_place(Args a, uint64_t pieces)
{
    place_body(image_of(a), a.buf, blockIdx.x, pieces, a.total);
}

hipError_t launch_scan(const uint32_t* in, uint64_t n, uint64_t* sums, uint64_t* out, hipStream_t st)
{
    const uint32_t nchunks = (uint32_t)((n + kScanChunk - 1) / kScanChunk);
    hipLaunchKernelGGL(k_jpeg_scan_sum, dim3(nchunks), dim3(256), 0, st, in, n, sums);
    hipLaunchKernelGGL(k_jpeg_scan_top, dim3(1), dim3(256), 0, st, sums, nchunks, out, n);
    hipLaunchKernelGGL(k_jpeg_scan_apply, dim3(nchunks), dim3(256), 0, st, in, n, (const uint64_t*)sums, out);
    return hipGetLastError();
}

hipError_t launch_encode(const Args& a, hipStream_t st)
{
    const Geom& g = a.g;
    const uint64_t pieces = raw_bound(g) / kPiece;
    if ((pieces + 255) / 256 > 0x7fffffffull)
        return hipErrorInvalidValue;
    const dim3 per_block((g.nblocks + 255) / 256), per_piece((uint32_t)((pieces + 255) / 256));
    hipLaunchKernelGGL(k_jpeg_transform, dim3((g.nblocks + 31) / 32), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_jpeg_size, per_block, dim3(256), 0, st, a);
    hipError_t e = launch_scan(a.buf.bits, g.nblocks, a.buf.sums, a.buf.bitoff, st);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_jpeg_interval_bytes, dim3((g.nint + 255) / 256), dim3(256), 0, st, a);
    e = launch_scan(a.buf.ibytes, g.nint, a.buf.sums, a.buf.ioff, st);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_jpeg_pack, per_block, dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_jpeg_count, per_piece, dim3(256), 0, st, a, pieces);
    e = launch_scan(a.buf.ffcnt, pieces, a.buf.sums, a.buf.ffoff, st);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_jpeg_place, per_piece, dim3(256), 0, st, a, pieces);
    return hipGetLastError();
}

}  // namespace jpeg
}  // namespace v1c
