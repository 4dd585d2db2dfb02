// kernels_jpeg.hip -- the device JPEG encoder's kernels: colour conversion, chroma downsampling, forward DCT and quantisation
// (transform); the coded bits of every block (size); bit packing of the intervals, most significant bit first (pack); the 0xFF
// bytes, and the stuffed intervals with their RSTm markers at their final offsets (count, place); the exclusive scans between
// them.  INTEGRATION.md section 7 has the stream contract, DESIGN.md section 13 the design.  A code object of its own: the remap
// and PNG kernels do not change with it.
//
// The standard Huffman tables are fixed, so the host takes no part between the kernels: they form one chain on the stream.  Every
// lane does a bounded amount of work whatever the restart interval, and nothing waits on another workgroup.  Words of the
// unstuffed stream that two blocks share are written with atomic ORs of disjoint bits into a zeroed buffer, words a block owns
// with plain stores, and every byte of the final stream is written exactly once: the result does not depend on any order.
#include <hip/hip_runtime.h>

#include "jpeg_kernels.hpp"

namespace v1c {
namespace jpeg {

// 1: pixels to quantised coefficients.  Eight lanes per block, one row (then one column) each; 32 blocks per workgroup.
__global__ __launch_bounds__(256) void k_jpeg_transform(Args a)
{
    __shared__ int tile[32][8][9];  // (rows padded to 9 words: the column pass reads without bank conflicts)
    __shared__ __attribute__((aligned(16))) int16_t zz[32 * 64];  // (stored from as 32-bit words)
    __shared__ uint16_t q[2][64];
    const int tid = threadIdx.x, blk = tid >> 3, r = tid & 7;
    if (tid < 128)
        q[tid >> 6][tid & 63] = a.tab->q[tid >> 6][tid & 63];
    const uint32_t b = blockIdx.x * 32u + (uint32_t)blk;
    const bool active = b < a.g.nblocks;
    BlockPos pos{};
    int d[8];
    if (active) {
        pos = block_pos(a.g, b);
#pragma unroll
        for (int c = 0; c < 8; c++)
            d[c] = plane_sample(a.img, a.pitch, a.g, pos.comp, pos.x0 + c, pos.y0 + r) - 128;
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
    const uint32_t nwords = min(32u, a.g.nblocks - blockIdx.x * 32u) * 32;
    uint32_t* dst = (uint32_t*)a.coef + (size_t)blockIdx.x * 1024;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t i = k * 256 + tid;
        if (i < nwords)
            dst[i] = ((const uint32_t*)zz)[i];
    }
}

// 2: the coded bits of every block, one block per lane.  The DC difference reads the predecessor's DC straight from the coefficient
// buffer: no block depends on another's result.
__global__ __launch_bounds__(256) void k_jpeg_size(Args a)
{
    __shared__ uint32_t lds[256 * kBlockWords];
    __shared__ uint32_t dc[2][16], ac[2][256];
    const int tid = threadIdx.x;
    const uint32_t b0 = blockIdx.x * 256u, b = b0 + tid;
    load_code_tables(dc, ac, a.tab, tid);
    stage_blocks(lds, a.coef, a.g.nblocks, b0, tid);
    __syncthreads();
    if (b >= a.g.nblocks)
        return;
    const uint32_t p = dc_predecessor(a.g, b);
    const int pred = p == b ? 0 : a.coef[(size_t)p * 64];
    const int t = block_pos(a.g, b).comp ? 1 : 0;
    uint32_t n = 0;
    encode_block(StagedBlock{(const int16_t*)(lds + tid * kBlockWords)}, pred, dc[t], ac[t], [&](uint32_t, int len) { n += (uint32_t)len; });
    a.bits[b] = n;
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

// 3: the bytes every interval takes before stuffing: its blocks' bits, padded to a whole byte
__global__ __launch_bounds__(256) void k_jpeg_interval_bytes(Args a)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.g.nint)
        return;
    const uint64_t f = (uint64_t)i * a.g.ibl, e = min(f + a.g.ibl, (uint64_t)a.g.nblocks);
    a.ibytes[i] = (uint32_t)((a.bitoff[e] - a.bitoff[f] + 7) >> 3);
}

// 4: every block's tokens at the block's bit of the unstuffed stream; an interval's last block adds the pad of 1-bits
__global__ __launch_bounds__(256) void k_jpeg_pack(Args a)
{
    __shared__ uint32_t lds[256 * kBlockWords];
    __shared__ uint32_t dc[2][16], ac[2][256];
    const int tid = threadIdx.x;
    const uint32_t b0 = blockIdx.x * 256u, b = b0 + tid;
    load_code_tables(dc, ac, a.tab, tid);
    stage_blocks(lds, a.coef, a.g.nblocks, b0, tid);
    __syncthreads();
    if (b >= a.g.nblocks)
        return;
    const uint32_t p = dc_predecessor(a.g, b);
    const int pred = p == b ? 0 : a.coef[(size_t)p * 64];
    const int t = block_pos(a.g, b).comp ? 1 : 0;
    const uint32_t iv = b / a.g.ibl;
    const uint64_t bit = 8 * a.ioff[iv] + (a.bitoff[b] - a.bitoff[(uint64_t)iv * a.g.ibl]);
    Packer pk((uint32_t*)a.raw, bit);
    encode_block(StagedBlock{(const int16_t*)(lds + tid * kBlockWords)}, pred, dc[t], ac[t], pk);
    if (b + 1 == a.g.nblocks || (b + 1) % a.g.ibl == 0) {
        const int pad = (int)((8 - ((bit + a.bits[b]) & 7)) & 7);
        if (pad)
            pk((1u << pad) - 1u, pad);
    }
    pk.finish();
}

// 5: the 0xFF bytes of every kPiece bytes of the unstuffed stream (zero behind its end: no bounds to mind)
__global__ __launch_bounds__(256) void k_jpeg_count(Args a, uint64_t pieces)
{
    const uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (p >= pieces)
        return;
    const uint4 v = ((const uint4*)a.raw)[p];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t n = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
        for (int s = 0; s < 32; s += 8)
            n += ((w[k] >> s) & 255u) == 255u ? 1u : 0u;
    a.ffcnt[p] = n;
}

// 6: every byte of the unstuffed stream at its final offset: behind the stuffing bytes and the markers in front of it.  A 0x00 follows
// every 0xFF, RSTm every interval but the last; the lane of the last byte writes the total.
__global__ __launch_bounds__(256) void k_jpeg_place(Args a, uint64_t pieces)
{
    const uint64_t p = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t total = a.ioff[a.g.nint], g0 = p * kPiece;
    if (p >= pieces || g0 >= total)
        return;
    // the interval of the piece's first byte: the last i with ioff[i] <= g0
    uint32_t lo = 0, hi = a.g.nint - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (a.ioff[mid] <= g0)
            lo = mid;
        else
            hi = mid - 1;
    }
    uint32_t iv = lo;
    uint64_t next = a.ioff[iv + 1], ff = a.ffoff[p];
    const uint4 v = ((const uint4*)a.raw)[p];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < kPiece; j++) {
        const uint64_t g = g0 + j;
        if (g >= total)
            break;
        if (g >= next) {  // (an interval has at least one byte: one step is enough)
            iv++;
            next = a.ioff[iv + 1];
        }
        const uint32_t byte = (w[j >> 2] >> ((j & 3) * 8)) & 255u;
        uint64_t at = g + ff + 2ull * iv;
        a.out[at++] = (uint8_t)byte;
        if (byte == 255u) {
            a.out[at++] = 0;
            ff++;
        }
        if (g + 1 == next && iv + 1 < a.g.nint) {
            a.out[at] = 0xff;
            a.out[at + 1] = (uint8_t)(0xd0 + (iv & 7u));
        }
        if (g + 1 == total)
            *a.total = at;
    }
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
    hipError_t e = launch_scan(a.bits, g.nblocks, a.sums, a.bitoff, st);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_jpeg_interval_bytes, dim3((g.nint + 255) / 256), dim3(256), 0, st, a);
    e = launch_scan(a.ibytes, g.nint, a.sums, a.ioff, st);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_jpeg_pack, per_block, dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_jpeg_count, per_piece, dim3(256), 0, st, a, pieces);
    e = launch_scan(a.ffcnt, pieces, a.sums, a.ffoff, st);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_jpeg_place, per_piece, dim3(256), 0, st, a, pieces);
    return hipGetLastError();
}

}  // namespace jpeg
}  // namespace v1c
