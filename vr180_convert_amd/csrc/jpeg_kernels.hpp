// jpeg_kernels.hpp -- the device code the JPEG encoder's two code objects share (kernels_jpeg.hip: one image; kernels_jpeg_batch.hip: a
// batch): the staging of a workgroup's blocks and of the code tables in LDS, the workgroup scan, the bit packer of a block, and the one
// text of the six stages (transform, size, interval_bytes, pack, count, place) as what a workgroup does for its Image (jpeg_batch.hpp),
// given the buffer set (Buffers, jpeg_launch.hpp) and its index within the image.  Every index in a body is relative to the image through
// jpeg_batch.hpp's helpers; the single call's Image has its regions at zero.  In an anonymous namespace: every code object has its own
// inlined copy.  profiles/jpeg_shared_bodies/ has both code objects before and after the stages were joined, and the timings.
#pragma once

#include <hip/hip_runtime.h>

#include "jpeg_batch.hpp"
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

// ---- the six stages ----------------------------------------------------------------------------------------------------------------------
// What one workgroup of a stage does for its image `im`, given the image's Tables, the buffer set and `wg`, its index among the image's
// workgroups of that stage.  Every index is relative to the image (jpeg_batch.hpp); the single call's image has its regions at zero.

// 1: pixels to quantised coefficients.  Eight lanes per block, one row (then one column) each; 32 blocks per workgroup.
// (tile's rows are padded to 9 words: the column pass reads without bank conflicts; zz is stored from as 32-bit words)
__device__ __forceinline__ void transform_body(const Image& im, const Tables* tab, const Buffers& buf, uint32_t wg, int (&tile)[32][8][9],
                                               int16_t (&zz)[32 * 64], uint16_t (&q)[2][64])
{
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
    uint32_t* dst = (uint32_t*)buf.coef + (size_t)(im.blk0 + (uint64_t)wg * 32) * 32;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t i = k * 256 + tid;
        if (i < nwords)
            dst[i] = ((const uint32_t*)zz)[i];
    }
}

// 2: the coded bits of every block, one block per lane.  The DC difference reads the predecessor's DC straight from the coefficient
// buffer: no block depends on another's result.
__device__ __forceinline__ void size_body(const Image& im, const Tables* tab, const Buffers& buf, uint32_t wg, uint32_t (&lds)[256 * kBlockWords],
                                          uint32_t (&dc)[2][16], uint32_t (&ac)[2][256])
{
    const int tid = threadIdx.x;
    const uint32_t b0 = wg * 256u, b = b0 + tid;
    load_code_tables(dc, ac, tab, tid);
    stage_blocks(lds, buf.coef + (size_t)im.blk0 * 64, im.g.nblocks, b0, tid);
    __syncthreads();
    if (b >= im.g.nblocks)
        return;
    const int pred = dc_prediction(im, buf.coef, b);
    const int t = block_pos(im.g, b).comp ? 1 : 0;
    uint32_t n = 0;
    encode_block(StagedBlock{(const int16_t*)(lds + tid * kBlockWords)}, pred, dc[t], ac[t], [&](uint32_t, int len) { n += (uint32_t)len; });
    buf.bits[im.blk0 + b] = n;
}

// 3: the bytes every interval takes before stuffing: its blocks' bits, padded to a whole byte
__device__ __forceinline__ void interval_bytes_body(const Image& im, const Buffers& buf, uint32_t wg)
{
    const uint32_t i = wg * 256u + threadIdx.x;
    if (i >= im.g.nint)
        return;
    buf.ibytes[im.int0 + i] = interval_bytes(im, buf.bitoff, i);
}

// 4: every block's tokens at the block's bit of its image's unstuffed stream; an interval's last block adds the pad of 1-bits
__device__ __forceinline__ void pack_body(const Image& im, const Tables* tab, const Buffers& buf, uint32_t wg, uint32_t (&lds)[256 * kBlockWords],
                                          uint32_t (&dc)[2][16], uint32_t (&ac)[2][256])
{
    const int tid = threadIdx.x;
    const uint32_t b0 = wg * 256u, b = b0 + tid;
    load_code_tables(dc, ac, tab, tid);
    stage_blocks(lds, buf.coef + (size_t)im.blk0 * 64, im.g.nblocks, b0, tid);
    __syncthreads();
    if (b >= im.g.nblocks)
        return;
    const int pred = dc_prediction(im, buf.coef, b);
    const int t = block_pos(im.g, b).comp ? 1 : 0;
    const uint64_t bit = block_bit(im, buf.bitoff, buf.ioff, b);
    Packer pk(buf.raw + (size_t)im.piece0 * (kPiece / 4), bit);
    encode_block(StagedBlock{(const int16_t*)(lds + tid * kBlockWords)}, pred, dc[t], ac[t], pk);
    if (b + 1 == im.g.nblocks || (b + 1) % im.g.ibl == 0) {
        const int pad = (int)((8 - ((bit + buf.bits[im.blk0 + b]) & 7)) & 7);
        if (pad)
            pk((1u << pad) - 1u, pad);
    }
    pk.finish();
}

// 5: the 0xFF bytes of every one of the `pieces` pieces of raw (zero behind every image's stream: no bounds to mind); needs no image,
// so wg counts over the whole of raw
__device__ __forceinline__ void count_body(const Buffers& buf, uint32_t wg, uint64_t pieces)
{
    const uint64_t p = (uint64_t)wg * 256u + threadIdx.x;
    if (p >= pieces)
        return;
    const uint4 v = ((const uint4*)buf.raw)[p];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t n = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
        for (int s = 0; s < 32; s += 8)
            n += ((w[k] >> s) & 255u) == 255u ? 1u : 0u;
    buf.ffcnt[p] = n;
}

// 6: every byte of the image's unstuffed stream at its final offset in the image's out region: behind the stuffing bytes and the markers
// in front of it.  A 0x00 follows every 0xFF, RSTm every interval but the last; the lane of the last byte writes the scan's size to *size.
// pieces: pieces_of(im.g), which the single call has from its host
__device__ __forceinline__ void place_body(const Image& im, const Buffers& buf, uint32_t wg, uint64_t pieces, uint64_t* size)
{
    const uint64_t p = (uint64_t)wg * 256u + threadIdx.x;
    const uint64_t total = interval_start(im, buf.ioff, im.g.nint), g0 = p * kPiece;
    if (p >= pieces || g0 >= total)
        return;
    // the interval of the piece's first byte: the last i of the image with interval_start(i) <= g0
    uint32_t lo = 0, hi = im.g.nint - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (interval_start(im, buf.ioff, mid) <= g0)
            lo = mid;
        else
            hi = mid - 1;
    }
    uint32_t iv = lo;
    uint64_t next = interval_start(im, buf.ioff, iv + 1), ff = ff_before(im, buf.ffoff, p);
    const uint4 v = ((const uint4*)buf.raw)[im.piece0 + p];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint8_t* out = buf.out + im.out0;
#pragma unroll
    for (int j = 0; j < kPiece; j++) {
        const uint64_t g = g0 + j;
        if (g >= total)
            break;
        if (g >= next) {  // (an interval has at least one byte: one step is enough)
            iv++;
            next = interval_start(im, buf.ioff, iv + 1);
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
            *size = at;
    }
}

}  // namespace

}  // namespace jpeg
}  // namespace v1c
