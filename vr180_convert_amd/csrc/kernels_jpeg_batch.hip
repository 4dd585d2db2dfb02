// kernels_jpeg_batch.hip -- the device JPEG encoder's kernels for a batch of images (v1c_jpeg_encode_batch): the kernels of
// kernels_jpeg.hip over flat work lists.  A workgroup finds its image by a bounded binary search over the images' first workgroups
// (file_of), takes that image's descriptor -- geometry, pitch, pointers, tables, and where its regions start in the concatenated
// buffers -- and does what the single call's workgroup of the same index within the image does, with image-relative indices.  The
// image is uniform per workgroup, so the descriptor lives in scalar registers and the tables are staged in LDS once per workgroup
// as there.  The three scans run once over the concatenation (launch_scan of kernels_jpeg.hip, as it is); jpeg_batch.hpp has the
// values that make a scanned entry the single call's.  DESIGN.md section 16 has the design.
//
// As in the single call, every lane's work is bounded whatever the restart interval -- and whatever the number of images: the image
// search is 32 halvings at the most --, nothing waits on another workgroup, and every byte of every file is written exactly once.  An
// image's raw region starts on a piece and is zeroed, so no word of it is shared with another image's blocks.
#include <hip/hip_runtime.h>

#include "jpeg_batch.hpp"
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

// 1: pixels to quantised coefficients, k_jpeg_transform's way: 32 blocks of one image per workgroup
__global__ __launch_bounds__(256) void k_jpegb_transform(Batch B)
{
    __shared__ int tile[32][8][9];
    __shared__ __attribute__((aligned(16))) int16_t zz[32 * 64];
    __shared__ uint16_t q[2][64];
    uint32_t wg;
    const Image im = B.im[image_of(B, kByTile, wg)];
    const Tables* tab = B.tabs + im.tab;
    const int tid = threadIdx.x, blk = tid >> 3, r = tid & 7;
    if (tid < 128)
        q[tid >> 6][tid & 63] = tab->q[tid >> 6][tid & 63];
    const uint32_t b = wg * 32u + (uint32_t)blk;
    const bool active = b < im.g.nblocks;
    BlockPos pos{};
    int d[8];
    if (active) {
        pos = block_pos(im.g, b);
#pragma unroll
        for (int c = 0; c < 8; c++)
            d[c] = plane_sample(im.img, im.pitch, im.g, pos.comp, pos.x0 + c, pos.y0 + r) - 128;
        fdct_pass<true>(d);
#pragma unroll
        for (int c = 0; c < 8; c++)
            tile[blk][r][c] = d[c];
    }
    __syncthreads();
    if (active) {
#pragma unroll
        for (int i = 0; i < 8; i++)
            d[i] = tile[blk][i][r];
        fdct_pass<false>(d);
        const int t = pos.comp ? 1 : 0;
#pragma unroll
        for (int i = 0; i < 8; i++)
            zz[blk * 64 + zigzag_of(i * 8 + r)] = (int16_t)quantise(d[i], q[t][i * 8 + r]);
    }
    __syncthreads();
    const uint32_t nwords = min(32u, im.g.nblocks - wg * 32u) * 32;
    uint32_t* dst = (uint32_t*)B.coef + (size_t)(im.blk0 + (uint64_t)wg * 32) * 32;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t i = k * 256 + tid;
        if (i < nwords)
            dst[i] = ((const uint32_t*)zz)[i];
    }
}

// 2: the coded bits of every block, one block per lane
__global__ __launch_bounds__(256) void k_jpegb_size(Batch B)
{
    __shared__ uint32_t lds[256 * kBlockWords];
    __shared__ uint32_t dc[2][16], ac[2][256];
    uint32_t wg;
    const Image im = B.im[image_of(B, kByBlock, wg)];
    const int tid = threadIdx.x;
    const uint32_t b0 = wg * 256u, b = b0 + tid;
    load_code_tables(dc, ac, B.tabs + im.tab, tid);
    stage_blocks(lds, B.coef + (size_t)im.blk0 * 64, im.g.nblocks, b0, tid);
    __syncthreads();
    if (b >= im.g.nblocks)
        return;
    const int pred = dc_prediction(im, B.coef, b);
    const int t = block_pos(im.g, b).comp ? 1 : 0;
    uint32_t n = 0;
    encode_block(StagedBlock{(const int16_t*)(lds + tid * kBlockWords)}, pred, dc[t], ac[t], [&](uint32_t, int len) { n += (uint32_t)len; });
    B.bits[im.blk0 + b] = n;
}

// 3: the bytes every interval takes before stuffing; the image's workgroups of the block list take 256 intervals each (an image
// has no more intervals than blocks)
__global__ __launch_bounds__(256) void k_jpegb_interval_bytes(Batch B)
{
    uint32_t wg;
    const Image im = B.im[image_of(B, kByBlock, wg)];
    const uint32_t i = wg * 256u + threadIdx.x;
    if (i >= im.g.nint)
        return;
    B.ibytes[im.int0 + i] = interval_bytes(im, B.bitoff, i);
}

// 4: every block's tokens at the block's bit of its image's unstuffed stream; an interval's last block adds the pad of 1-bits
__global__ __launch_bounds__(256) void k_jpegb_pack(Batch B)
{
    __shared__ uint32_t lds[256 * kBlockWords];
    __shared__ uint32_t dc[2][16], ac[2][256];
    uint32_t wg;
    const Image im = B.im[image_of(B, kByBlock, wg)];
    const int tid = threadIdx.x;
    const uint32_t b0 = wg * 256u, b = b0 + tid;
    load_code_tables(dc, ac, B.tabs + im.tab, tid);
    stage_blocks(lds, B.coef + (size_t)im.blk0 * 64, im.g.nblocks, b0, tid);
    __syncthreads();
    if (b >= im.g.nblocks)
        return;
    const int pred = dc_prediction(im, B.coef, b);
    const int t = block_pos(im.g, b).comp ? 1 : 0;
    const uint64_t bit = block_bit(im, B.bitoff, B.ioff, b);
    Packer pk(B.raw + (size_t)im.piece0 * (kPiece / 4), bit);
    encode_block(StagedBlock{(const int16_t*)(lds + tid * kBlockWords)}, pred, dc[t], ac[t], pk);
    if (b + 1 == im.g.nblocks || (b + 1) % im.g.ibl == 0) {
        const int pad = (int)((8 - ((bit + B.bits[im.blk0 + b]) & 7)) & 7);
        if (pad)
            pk((1u << pad) - 1u, pad);
    }
    pk.finish();
}

// 5: the 0xFF bytes of every piece of the concatenated raw (zero behind every image's stream); needs no image
__global__ __launch_bounds__(256) void k_jpegb_count(Batch B)
{
    const uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (p >= B.t.pieces)
        return;
    const uint4 v = ((const uint4*)B.raw)[p];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t n = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
        for (int s = 0; s < 32; s += 8)
            n += ((w[k] >> s) & 255u) == 255u ? 1u : 0u;
    B.ffcnt[p] = n;
}

// 6: every byte of an image's unstuffed stream at its final offset in the image's out region; the lane of the image's last byte
// writes the image's size
__global__ __launch_bounds__(256) void k_jpegb_place(Batch B)
{
    uint32_t wg;
    const uint32_t f = image_of(B, kByPiece, wg);
    const Image im = B.im[f];
    const uint64_t p = (uint64_t)wg * 256u + threadIdx.x;
    const uint64_t total = interval_start(im, B.ioff, im.g.nint), g0 = p * kPiece;
    if (p >= pieces_of(im.g) || g0 >= total)
        return;
    // the interval of the piece's first byte: the last i of the image with interval_start(i) <= g0
    uint32_t lo = 0, hi = im.g.nint - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (interval_start(im, B.ioff, mid) <= g0)
            lo = mid;
        else
            hi = mid - 1;
    }
    uint32_t iv = lo;
    uint64_t next = interval_start(im, B.ioff, iv + 1), ff = ff_before(im, B.ffoff, p);
    const uint4 v = ((const uint4*)B.raw)[im.piece0 + p];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint8_t* out = B.out + im.out0;
#pragma unroll
    for (int j = 0; j < kPiece; j++) {
        const uint64_t g = g0 + j;
        if (g >= total)
            break;
        if (g >= next) {  // (an interval has at least one byte: one step is enough)
            iv++;
            next = interval_start(im, B.ioff, iv + 1);
        }
        const uint32_t byte = (w[j >> 2] >> ((j & 3) * 8)) & 255u;
        uint64_t at = g + ff + 2ull * iv;
        out[at++] = (uint8_t)byte;
        if (byte == 255u) {
            out[at++] = 0;
            ff++;
        }
        if (g + 1 == next && iv + 1 < im.g.nint) {
            out[at] = 0xff;
            out[at + 1] = rst_marker(iv);
        }
        if (g + 1 == total)
            B.sizes[f] = at;
    }
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
    hipError_t e = launch_scan(b.bits, b.t.nblocks, b.sums, b.bitoff, st);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_jpegb_interval_bytes, dim3(groups[kByBlock]), dim3(256), 0, st, b);
    e = launch_scan(b.ibytes, b.t.nint, b.sums, b.ioff, st);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_jpegb_pack, dim3(groups[kByBlock]), dim3(256), 0, st, b);
    hipLaunchKernelGGL(k_jpegb_count, dim3((uint32_t)((b.t.pieces + 255) / 256)), dim3(256), 0, st, b);
    e = launch_scan(b.ffcnt, b.t.pieces, b.sums, b.ffoff, st);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_jpegb_place, dim3(groups[kByPiece]), dim3(256), 0, st, b);
    return hipGetLastError();
}

}  // namespace jpeg
}  // namespace v1c
