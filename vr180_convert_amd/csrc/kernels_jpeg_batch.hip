// kernels_jpeg_batch.hip -- the device JPEG encoder's kernels for a batch of images (v1c_jpeg_encode_batch): the kernels of
// kernels_jpeg.hip over flat work lists.  A workgroup finds its image by a bounded binary search over the images' first workgroups
// (file_of), takes that image's descriptor -- geometry, pitch, pointers, tables, and where its regions start in the concatenated
// buffers -- and calls the stage's body (jpeg_kernels.hpp) with it and its index within the image: the body the single call's kernel
// calls with an image whose regions start at zero.  The image is uniform per workgroup, so the descriptor lives in scalar registers
// and the tables are staged in LDS once per workgroup.  The three scans run once over the concatenation (launch_scan of
// kernels_jpeg.hip, as it is); jpeg_batch.hpp has the values that make a scanned entry the image's own.  DESIGN.md section 16 has the
// design.
//
// As in the single call, every lane's work is bounded whatever the restart interval -- and whatever the number of images: the image
// search is 32 halvings at the most --, nothing waits on another workgroup, and every byte of every file is written exactly once.  An
// image's raw region starts on a piece and is zeroed, so no word of it is shared with another image's blocks.
#include <hip/hip_runtime.h>

#include "jpeg_kernels.hpp"

namespace v1c {
namespace jpeg {

namespace {

// the workgroup's image and, through wg, its index within the image
__device__ __forceinline__ uint32_t image_of(const Batch& b, int list, uint32_t& wg)
{
    const uint32_t* first = b.first + (size_t)list * (b.n + 1);
    const uint32_t f = file_of(first, b.n, blockIdx.x);
    wg = blockIdx.x - first[f];
    return f;
}

}  // namespace

__global__ __launch_bounds__(256) void k_jpegb_transform(Batch B)
{
    __shared__ int tile[32][8][9];
    __shared__ __attribute__((aligned(16))) int16_t zz[32 * 64];
    __shared__ uint16_t q[2][64];
    uint32_t wg;
    const Image im = B.im[image_of(B, kByTile, wg)];
    transform_body(im, B.tabs + im.tab, B.buf, wg, tile, zz, q);
}

__global__ __launch_bounds__(256) void k_jpegb_size(Batch B)
{
    __shared__ uint32_t lds[256 * kBlockWords];
    __shared__ uint32_t dc[2][16], ac[2][256];
    uint32_t wg;
    const Image im = B.im[image_of(B, kByBlock, wg)];
    size_body(im, B.tabs + im.tab, B.buf, wg, lds, dc, ac);
}

// the image's workgroups of the block list take 256 intervals each (an image has no more intervals than blocks)
__global__ __launch_bounds__(256) void k_jpegb_interval_bytes(Batch B)
{
    uint32_t wg;
    const Image im = B.im[image_of(B, kByBlock, wg)];
    interval_bytes_body(im, B.buf, wg);
}

__global__ __launch_bounds__(256) void k_jpegb_pack(Batch B)
{
    __shared__ uint32_t lds[256 * kBlockWords];
    __shared__ uint32_t dc[2][16], ac[2][256];
    uint32_t wg;
    const Image im = B.im[image_of(B, kByBlock, wg)];
    pack_body(im, B.tabs + im.tab, B.buf, wg, lds, dc, ac);
}

// over the concatenated raw
__global__ __launch_bounds__(256) void k_jpegb_count(Batch B)
{
    count_body(B.buf, blockIdx.x, B.t.pieces);
}

__global__ __launch_bounds__(256) void k_jpegb_place(Batch B)
{
    uint32_t wg;
    const uint32_t f = image_of(B, kByPiece, wg);
    const Image im = B.im[f];
    place_body(im, B.buf, wg, pieces_of(im.g), &B.sizes[f]);
}

hipError_t launch_encode_batch(const Batch& b, const uint32_t* first_host, hipStream_t st)
{
    uint32_t groups[kWorkLists];
    for (int l = 0; l < kWorkLists; l++) {
        groups[l] = first_host[(size_t)l * (b.n + 1) + b.n];
        if (groups[l] == 0 || groups[l] > 0x7fffffffu)
            return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(k_jpegb_transform, dim3(groups[kByTile]), dim3(256), 0, st, b);
    hipLaunchKernelGGL(k_jpegb_size, dim3(groups[kByBlock]), dim3(256), 0, st, b);
    hipError_t e = launch_scan(b.buf.bits, b.t.nblocks, b.buf.sums, b.buf.bitoff, st);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_jpegb_interval_bytes, dim3(groups[kByBlock]), dim3(256), 0, st, b);
    e = launch_scan(b.buf.ibytes, b.t.nint, b.buf.sums, b.buf.ioff, st);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_jpegb_pack, dim3(groups[kByBlock]), dim3(256), 0, st, b);
    hipLaunchKernelGGL(k_jpegb_count, dim3((uint32_t)((b.t.pieces + 255) / 256)), dim3(256), 0, st, b);
    e = launch_scan(b.buf.ffcnt, b.t.pieces, b.buf.sums, b.buf.ffoff, st);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_jpegb_place, dim3(groups[kByPiece]), dim3(256), 0, st, b);
    return hipGetLastError();
}

}  // namespace jpeg
}  // namespace v1c
