// kernels_jpegxc.hip -- the lossless JPEG transcoder's kernel and its launchers (v1c_jpeg_transcode, jpegxc.hip): between the device
// decoder's last Huffman pass and the device encoder's size stage, k_jxc_gather copies the blocks of an output -- rectangles of the
// source's MCUs -- from the decoder's coefficient store into the encoder's, with the DC a value.  No inverse DCT, no pixels, no forward
// DCT: every coefficient is carried over as it is.  Everything else a transcode runs is the two codecs' own kernels, launched from here
// as they are -- the decoder's DC gather (kernels_jpegdec.hip), the scans (kernels_jpeg.hip), the batch encoder's interval, count and
// place stages (kernels_jpeg_batch.hip) and the optimised tables' builder (kernels_jpeg_opt.hip) -- but for the three stages that ask
// which component a block belongs to and which block its DC is predicted from: size, pack and the histograms.  The encoder's
// answer (jpeg_core.hpp) knows MCUs of one block per component and of four luma blocks; a 4:2:2 file has two, so k_jxc_size,
// k_jxc_pack and k_jxc_hist here are those stages over jpegxc_core.hpp's answer for any MCU, built from the encoder's own parts
// (staging, code tables, the coder of a block, the packer: jpeg_kernels.hpp, jpeg_opt_kernels.hpp).  INTEGRATION.md section 9 has the contract,
// DESIGN.md section 19 the design.  A code object of its own: the codecs' code objects do not change with it.
//
// Nothing waits on another workgroup and the region search is bounded by kMaxRegions.  A block is 128 bytes: eight lanes move it as
// eight 16-byte words, so a wave reads and writes eight whole blocks per instruction, the writes contiguous over the wave.
#include <hip/hip_runtime.h>

#include "jpegxc_launch.hpp"

namespace v1c {

// the codecs' kernels (kernels_jpegdec.hip, kernels_jpeg_batch.hip, kernels_jpeg_opt.hip)
namespace jpegdec {
__global__ void k_jdec_dcgather(Args a);
}
namespace jpeg {
__global__ void k_jpegb_interval_bytes(Batch B);
__global__ void k_jpegb_count(Batch B);
__global__ void k_jpegb_place(Batch B);
__global__ void k_jpego_build(OptBatch O);
}  // namespace jpeg

namespace jpegxc {

// 32 blocks per workgroup, eight lanes each.  The region list comes with the kernel's arguments: constant memory, read with scalar
// loads (the list and the loop over it are the same for every lane).
__global__ __launch_bounds__(256) void k_jxc_gather(GatherArgs a)
{
    const uint32_t b = blockIdx.x * 32u + (threadIdx.x >> 3), part = threadIdx.x & 7u;
    if (b >= a.dst_nblocks)
        return;
    const uint32_t sb = source_block(a.regions, a.sg.mcux, a.dst_mcux, a.sg.bpm, b);
    uint4 v = make_uint4(0u, 0u, 0u, 0u);  // (a block no region holds: the host refuses such an output before any launch)
    int first = 0;                         // the lane's first coefficient as it is judged: the DC before it is cut to the 16 bits stored
    if (sb != kNone) {
        v = ((const uint4*)a.src)[(size_t)sb * 8 + part];
        first = (int16_t)(v.x & 0xffffu);
        if (part == 0) {
            first = dc_value(a.sg, a.dcoff, sb);
            v.x = (v.x & 0xffff0000u) | (uint32_t)(uint16_t)first;
        }
    }
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    bool ok = codable(first, part == 0) & codable((int16_t)(w[0] >> 16), false);
#pragma unroll
    for (int k = 1; k < 4; k++) {
        ok &= codable((int16_t)(w[k] & 0xffffu), false);
        ok &= codable((int16_t)(w[k] >> 16), false);
    }
    ((uint4*)a.dst)[(size_t)b * 8 + part] = v;
    if (!ok)
        atomicOr(a.flag, 1u);
}

// ---- the three stages that read a block's component and its DC predecessor: jpeg_kernels.hpp's size_body and pack_body and
// jpeg_opt_kernels.hpp's hist_body with jpegxc_core.hpp's table_class and xc_prediction in place of the encoder's ---------------------------

namespace {

// the workgroup's image in the block list and, through wg, its index within the image
__device__ __forceinline__ uint32_t image_of(const jpeg::Batch& B, uint32_t& wg)
{
    const uint32_t* first = B.first + (size_t)jpeg::kByBlock * (B.n + 1);
    const uint32_t f = jpeg::file_of(first, B.n, blockIdx.x);
    wg = blockIdx.x - first[f];
    return f;
}

}  // namespace

__global__ __launch_bounds__(256) void k_jxc_size(jpeg::Batch B)
{
    using namespace jpeg;
    __shared__ uint32_t lds[256 * kBlockWords];
    __shared__ uint32_t dc[2][16], ac[2][256];
    uint32_t wg;
    const Image im = B.im[image_of(B, wg)];
    const int tid = threadIdx.x;
    const uint32_t b0 = wg * 256u, b = b0 + tid;
    load_code_tables(dc, ac, B.tabs + im.tab, tid);
    stage_blocks(lds, B.buf.coef + (size_t)im.blk0 * 64, im.g.nblocks, b0, tid);
    __syncthreads();
    if (b >= im.g.nblocks)
        return;
    const int pred = xc_prediction(im.g, B.buf.coef, im.blk0, b), t = table_class(im.g, b);
    uint32_t n = 0;
    encode_block(StagedBlock{(const int16_t*)(lds + tid * kBlockWords)}, pred, dc[t], ac[t], [&](uint32_t, int len) { n += (uint32_t)len; });
    B.buf.bits[im.blk0 + b] = n;
}

__global__ __launch_bounds__(256) void k_jxc_pack(jpeg::Batch B)
{
    using namespace jpeg;
    __shared__ uint32_t lds[256 * kBlockWords];
    __shared__ uint32_t dc[2][16], ac[2][256];
    uint32_t wg;
    const Image im = B.im[image_of(B, wg)];
    const int tid = threadIdx.x;
    const uint32_t b0 = wg * 256u, b = b0 + tid;
    load_code_tables(dc, ac, B.tabs + im.tab, tid);
    stage_blocks(lds, B.buf.coef + (size_t)im.blk0 * 64, im.g.nblocks, b0, tid);
    __syncthreads();
    if (b >= im.g.nblocks)
        return;
    const int pred = xc_prediction(im.g, B.buf.coef, im.blk0, b), t = table_class(im.g, b);
    const uint64_t bit = block_bit(im, B.buf.bitoff, B.buf.ioff, b);
    Packer pk(B.buf.raw + (size_t)im.piece0 * (kPiece / 4), bit);
    encode_block(StagedBlock{(const int16_t*)(lds + tid * kBlockWords)}, pred, dc[t], ac[t], pk);
    if (b + 1 == im.g.nblocks || (b + 1) % im.g.ibl == 0) {
        const int pad = (int)((8 - ((bit + B.buf.bits[im.blk0 + b]) & 7)) & 7);
        if (pad)
            pk((1u << pad) - 1u, pad);
    }
    pk.finish();
}

// over the block list: a workgroup of an output with the Annex K tables has nothing to do
__global__ __launch_bounds__(256) void k_jxc_hist(jpeg::Batch B, jpeg::OptBatch O)
{
    using namespace jpeg;
    __shared__ uint32_t lds[256 * kBlockWords];
    __shared__ uint32_t identity[256], cnt[kHistWords];
    uint32_t wg;
    const uint32_t f = image_of(B, wg);
    const int32_t slot = O.slot_of[f];
    if (slot < 0)
        return;
    const Image im = B.im[f];
    const int tid = threadIdx.x;
    const uint32_t b0 = wg * 256u, b = b0 + tid;
    identity[tid] = identity_entry(tid);
    for (int i = tid; i < kHistWords; i += 256)
        cnt[i] = 0;
    stage_blocks(lds, B.buf.coef + (size_t)im.blk0 * 64, im.g.nblocks, b0, tid);
    __syncthreads();
    if (b < im.g.nblocks) {
        const int pred = xc_prediction(im.g, B.buf.coef, im.blk0, b), t = table_class(im.g, b);
        block_symbols(StagedBlock{(const int16_t*)(lds + tid * kBlockWords)}, pred, identity,
                      [&](bool isdc, int symbol) { atomicAdd(&cnt[hist_word(isdc, t, symbol)], 1u); });
    }
    __syncthreads();
    Hist* hist = O.hist + slot;
    for (int i = tid; i < kHistWords; i += 256) {
        const uint32_t n = cnt[i];
        if (!n)
            continue;
        const bool isdc = i < 32;
        const int t = isdc ? i >> 4 : (i - 32) >> 8, symbol = isdc ? i & 15 : (i - 32) & 255;
        atomicAdd((unsigned long long*)&hist->n[hist_of(isdc, t)][symbol], (unsigned long long)n);
    }
}

hipError_t launch_dc(const jpegdec::Args& a, hipStream_t st)
{
    hipLaunchKernelGGL(jpegdec::k_jdec_dcgather, dim3((a.g.nblocks + 255) / 256), dim3(256), 0, st, a);
    return jpeg::launch_scan(a.dcd, a.g.nblocks, a.sums, a.dcoff, st);
}

hipError_t launch_gather(const GatherArgs& a, hipStream_t st)
{
    hipLaunchKernelGGL(k_jxc_gather, dim3((a.dst_nblocks + 31) / 32), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_encode_coef(const jpeg::Batch& b, const jpeg::OptBatch* o, const uint32_t* first_host, hipStream_t st)
{
    using namespace jpeg;
    uint32_t groups[kWorkLists];
    for (int l = 0; l < kWorkLists; l++) {
        groups[l] = first_host[(size_t)l * (b.n + 1) + b.n];
        if (groups[l] == 0 || groups[l] > 0x7fffffffu)
            return hipErrorInvalidValue;
    }
    if (o) {
        if (o->nslots == 0 || o->nslots > 0x7fffffffu / kOptTables)
            return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_jxc_hist, dim3(groups[kByBlock]), dim3(256), 0, st, b, *o);
        hipLaunchKernelGGL(k_jpego_build, dim3(o->nslots * kOptTables), dim3(64), 0, st, *o);
    }
    hipLaunchKernelGGL(k_jxc_size, dim3(groups[kByBlock]), dim3(256), 0, st, b);
    hipError_t e = launch_scan(b.buf.bits, b.t.nblocks, b.buf.sums, b.buf.bitoff, st);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_jpegb_interval_bytes, dim3(groups[kByBlock]), dim3(256), 0, st, b);
    e = launch_scan(b.buf.ibytes, b.t.nint, b.buf.sums, b.buf.ioff, st);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_jxc_pack, dim3(groups[kByBlock]), dim3(256), 0, st, b);
    hipLaunchKernelGGL(k_jpegb_count, dim3((uint32_t)((b.t.pieces + 255) / 256)), dim3(256), 0, st, b);
    e = launch_scan(b.buf.ffcnt, b.t.pieces, b.buf.sums, b.buf.ffoff, st);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_jpegb_place, dim3(groups[kByPiece]), dim3(256), 0, st, b);
    return hipGetLastError();
}

}  // namespace jpegxc
}  // namespace v1c
