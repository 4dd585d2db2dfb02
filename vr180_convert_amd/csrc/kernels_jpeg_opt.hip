// kernels_jpeg_opt.hip -- the kernels of the optimised Huffman tables (v1c_jpeg_encode_opt, v1c_jpeg_encode_batch_opt): the symbol
// histograms of every optimising image of a chunk (k_jpego_hist) and the tables they give (k_jpego_build), run between the transform
// and the size stage of the batch's chain (kernels_jpeg_batch.hip), whose kernels are launched from here as they are: the size, pack
// and place stages only see Tables that the device filled.  The single optimising call is a chunk of one image.  DESIGN.md section 17
// has the design, INTEGRATION.md section 7 the procedure.  A code object of its own: a plain encode does not load it, and the other
// code objects do not change with it.
//
// Counting is order-free (atomic adds of integers) and the builder is integer arithmetic on the counts: the tables, so the file, are a
// pure function of the pixels and the parameters.
#include <hip/hip_runtime.h>

#include "jpeg_opt_kernels.hpp"

namespace v1c {
namespace jpeg {

// the batch's stages (kernels_jpeg_batch.hip)
__global__ void k_jpegb_transform(Batch B);
__global__ void k_jpegb_size(Batch B);
__global__ void k_jpegb_interval_bytes(Batch B);
__global__ void k_jpegb_pack(Batch B);
__global__ void k_jpegb_count(Batch B);
__global__ void k_jpegb_place(Batch B);

// over the block list: a workgroup of an image with the Annex K tables has nothing to do
__global__ __launch_bounds__(256) void k_jpego_hist(Batch B, OptBatch O)
{
    __shared__ uint32_t lds[256 * kBlockWords];
    __shared__ uint32_t identity[256], cnt[kHistWords];
    const uint32_t* first = B.first + (size_t)kByBlock * (B.n + 1);
    const uint32_t f = file_of(first, B.n, blockIdx.x);
    const int32_t slot = O.slot_of[f];
    if (slot < 0)
        return;
    hist_body(B.im[f], B.buf, blockIdx.x - first[f], O.hist + slot, lds, identity, cnt);
}

// one wave per slot and table
__global__ __launch_bounds__(64) void k_jpego_build(OptBatch O)
{
    __shared__ BuildScratch s;
    build_body(O, blockIdx.x / kOptTables, (int)(blockIdx.x % kOptTables), s);
}

hipError_t launch_encode_batch_opt(const Batch& b, const OptBatch& o, const uint32_t* first_host, hipStream_t st)
{
    uint32_t groups[kWorkLists];
    for (int l = 0; l < kWorkLists; l++) {
        groups[l] = first_host[(size_t)l * (b.n + 1) + b.n];
        if (groups[l] == 0 || groups[l] > 0x7fffffffu)
            return hipErrorInvalidValue;
    }
    if (o.nslots == 0 || o.nslots > 0x7fffffffu / kOptTables)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_jpegb_transform, dim3(groups[kByTile]), dim3(256), 0, st, b);
    hipLaunchKernelGGL(k_jpego_hist, dim3(groups[kByBlock]), dim3(256), 0, st, b, o);
    hipLaunchKernelGGL(k_jpego_build, dim3(o.nslots * kOptTables), dim3(64), 0, st, o);
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
