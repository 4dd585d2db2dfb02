// jpegdec_kernels.hpp -- what one workgroup of every kernel of the device JPEG decoder does, given its file's Args BY REFERENCE and its
// index within the file: the one text of the eight stages.  kernels_jpegdec.hip calls the bodies with the kernel's own parameter and
// blockIdx.x; kernels_jpegdec_batch.hip first looks up the workgroup's file (jpegdec_batch.hpp) and calls them with that file's Args in
// device memory and the index within the file.  The caller names the flag words and declares the LDS.  A body binds the Args it is
// given and never copies them: a by-value copy sends k_jdec_sync to 392 bytes of scratch per lane (the run-time index into exit[r & 1]).
// The per-lane arithmetic is jpegdec_core.hpp's.  profiles/jpeg_shared_bodies/ has the single-file code object before and after it was
// built from these bodies, and the timings; tests/test_gpu_jpegdec_batch.py holds batch and single call to each other sample for sample,
// report for report.  Device code only.
#pragma once

#include <hip/hip_runtime.h>

#include "jpegdec_launch.hpp"

namespace v1c {
namespace jpegdec {

constexpr int kTableWords = (int)(8 * sizeof(Table) / 4);

// the eight Huffman tables into LDS (Tables: dc[4] and ac[4] lie back to back)
__device__ inline void load_tables(Table* t, const Tables* src, int tid)
{
    const uint32_t* s = (const uint32_t*)&src->dc[0];
    uint32_t* d = (uint32_t*)t;
    for (int i = tid; i < kTableWords; i += 256)
        d[i] = s[i];
}

__device__ inline TablePair pair_of(const Geom& g, const Table* t)
{
    TablePair tp{t, t + 4, 0, 0};
    const uint32_t cd = g.td[1] | g.td[2] << 4, ca = g.ta[1] | g.ta[2] << 4;  // chroma: the blocks behind the ny luma ones
    for (uint32_t c = 0; c < 4; c++) {
        tp.dcsel |= (c < g.ny ? (uint32_t)g.td[0] : 0u) << (4 * c);
        tp.acsel |= (c < g.ny ? (uint32_t)g.ta[0] : 0u) << (4 * c);
    }
    if (g.nc == 3) {
        tp.dcsel |= cd << (4 * g.ny);
        tp.acsel |= ca << (4 * g.ny);
    }
    return tp;
}

struct Sub {
    uint32_t k, start, end, E;  // segment; first bit, end bit, the segment's end bit
    bool first, last;           // of its segment
};

__device__ inline Sub sub_of(const Args& a, uint32_t i)
{
    uint32_t lo = 0, hi = a.g.nseg - 1;
    for (int it = 0; it < 32 && lo < hi; it++) {  // the last k with subfirst[k] <= i
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (a.subfirst[mid] <= i)
            lo = mid;
        else
            hi = mid - 1;
    }
    Sub s;
    s.k = lo;
    s.E = 8 * a.segoff[lo + 1];
    const uint32_t j = i - a.subfirst[lo];
    s.start = 8 * a.segoff[lo] + j * a.S;
    s.end = min(s.start + a.S, s.E);
    s.first = j == 0;
    s.last = i + 1 == a.subfirst[lo + 1];
    return s;
}

// 1: the bytes every piece of the stuffed scan drops
__device__ __forceinline__ void count_body(const Args& a, uint32_t wg)
{
    const uint32_t p = wg * 256u + threadIdx.x;
    if (p >= a.pieces)
        return;
    const uint4 v = ((const uint4*)a.scan)[p];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t prev = p ? a.scan[(size_t)p * kPiece - 1] : 0u, n = 0;
    const uint32_t after = a.scan[(size_t)p * kPiece + kPiece];
#pragma unroll
    for (int j = 0; j < kPiece; j++) {
        const uint32_t cur = (w[j >> 2] >> ((j & 3) * 8)) & 255u;
        const uint32_t next = j + 1 < kPiece ? (w[(j + 1) >> 2] >> (((j + 1) & 3) * 8)) & 255u : after;
        n += (p * kPiece + j < a.scan_len && dropped(prev, cur, next)) ? 1u : 0u;
        prev = cur;
    }
    a.drop[p] = n;
}

// 2: every kept byte at its place in the unstuffed stream
__device__ __forceinline__ void place_body(const Args& a, uint32_t wg)
{
    const uint32_t p = wg * 256u + threadIdx.x;
    if (p >= a.pieces)
        return;
    const uint4 v = ((const uint4*)a.scan)[p];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t prev = p ? a.scan[(size_t)p * kPiece - 1] : 0u;
    const uint32_t after = a.scan[(size_t)p * kPiece + kPiece];
    uint8_t* dst = (uint8_t*)a.u + ((uint64_t)p * kPiece - a.dropoff[p]);  // (at most the piece's own offset: inside a.u)
#pragma unroll
    for (int j = 0; j < kPiece; j++) {
        const uint32_t cur = (w[j >> 2] >> ((j & 3) * 8)) & 255u;
        const uint32_t next = j + 1 < kPiece ? (w[(j + 1) >> 2] >> (((j + 1) & 3) * 8)) & 255u : after;
        if (p * kPiece + j < a.scan_len && !dropped(prev, cur, next))
            *dst++ = (uint8_t)cur;
        prev = cur;
    }
}

// 3: before the first round: what F_i "gave" is the grid state of the subsequence behind it, and no entry state was computed for
__device__ __forceinline__ void init_body(const Args& a, uint32_t wg)
{
    const uint32_t i = wg * 256u + threadIdx.x;
    if (i >= a.nsub)
        return;
    const Sub s = sub_of(a, i);
    a.exit[0][i] = State{s.end, 0u};
    a.last[i] = State{0xffffffffu, 0xffffffffu};
    a.count[i] = 0;
}

// 4: one round.  A lane whose entry state is the one it last computed for passes its result on; the others run F_i.  A changed entry
// state of any subsequence raises this round's flag *raise; the file's first lane clears the next round's, *clear, which nobody reads or
// raises before this kernel has ended.  t: the file's tables in LDS.
__device__ __forceinline__ void sync_body(const Args& a, uint32_t wg, uint32_t r, const Table* t, uint32_t* raise, uint32_t* clear)
{
    const uint32_t i = wg * 256u + threadIdx.x;
    if (i == 0)
        *clear = 0;
    if (i >= a.nsub)
        return;
    const State *in = a.exit[(r - 1) & 1u];
    State* out = a.exit[r & 1u];
    const Sub s = sub_of(a, i);
    const State e = s.first ? State{s.start, 0u} : in[i - 1];
    const State was = in[i];
    if (e == a.last[i]) {
        out[i] = was;
        return;
    }
    State x = e;
    const uint32_t n = decode_span<false>(a.u, pair_of(a.g, t), a.g.bpm, x, s.end, s.E, nullptr, 0, 0, nullptr);
    a.last[i] = e;
    a.count[i] = n;
    out[i] = x;
    if (!s.last && !(x == was))
        *raise = 1;
}

// 5: the last pass: every subsequence from its true entry state into the coefficients, the DC still a difference.  Only this pass
// judges the stream: an invalid code, a run past 63, a symbol past the segment's end, a segment whose blocks are not the geometry's.
// r: the file's last round; *verdict gets the first error bit.
__device__ __forceinline__ void write_body(const Args& a, uint32_t wg, uint32_t r, const Table* t, uint32_t* verdict)
{
    const uint32_t i = wg * 256u + threadIdx.x;
    if (i >= a.nsub)
        return;
    const State* fin = a.exit[r & 1u];
    const Sub s = sub_of(a, i);
    State e = s.first ? State{s.start, 0u} : fin[i - 1];
    const uint32_t i0 = a.subfirst[s.k], b0 = s.k * a.g.ibl, bq = min(b0 + a.g.ibl, a.g.nblocks);
    const uint64_t done = a.first[i] - a.first[i0];
    const uint32_t b = done < bq - b0 ? b0 + (uint32_t)done : bq;
    uint32_t err = kNoError;
    decode_span<true>(a.u, pair_of(a.g, t), a.g.bpm, e, s.end, s.E, a.coef, b, bq, &err);
    if (s.first && a.first[a.subfirst[s.k + 1]] - a.first[i0] != bq - b0)
        err = min(err, s.start);
    if (err != kNoError)
        atomicMin(verdict, err);
}

// 6: the DC differences in the order their scan runs over: all blocks of Y, of Cb, of Cr
__device__ __forceinline__ void dcgather_body(const Args& a, uint32_t wg)
{
    const uint32_t b = wg * 256u + threadIdx.x;
    if (b >= a.g.nblocks)
        return;
    uint32_t pos, pos0;
    dc_pos(a.g, b, pos, pos0);
    a.dcd[pos] = (uint32_t)(int)a.coef[(size_t)b * 64];
}

// 7: coefficients to samples.  Eight lanes per block, one column (then one row) each; 32 blocks per workgroup.
// (tile's rows are padded to 9 words: the row pass reads without bank conflicts)
__device__ __forceinline__ void idct_body(const Args& a, uint32_t wg, int (&tile)[32][8][9], int16_t (&zz)[32 * 64], uint16_t (&q)[4][64])
{
    const int tid = threadIdx.x, blk = tid >> 3, r = tid & 7;
    q[tid >> 6][tid & 63] = a.tab->q[tid >> 6][tid & 63];
    const uint32_t nwords = min(32u, a.g.nblocks - wg * 32u) * 32;
    const uint32_t* src = (const uint32_t*)a.coef + (size_t)wg * 1024;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t i = k * 256 + tid;
        if (i < nwords)
            ((uint32_t*)zz)[i] = src[i];
    }
    __syncthreads();
    const uint32_t b = wg * 32u + (uint32_t)blk;
    const bool active = b < a.g.nblocks;
    BlockPos pos{};
    int d[8];
    if (active) {
        pos = block_pos(a.g, b);
        const int tq = pos.comp == 0 ? a.g.tq[0] : pos.comp == 1 ? a.g.tq[1] : a.g.tq[2];
#pragma unroll
        for (int i = 0; i < 8; i++)
            d[i] = dequantise(zz[blk * 64 + zigzag_of(i * 8 + r)], q[tq][i * 8 + r]);
        if (r == 0) {
            uint32_t at, at0;
            dc_pos(a.g, b, at, at0);
            d[0] = dequantise((int16_t)(uint32_t)(a.dcoff[at + 1] - a.dcoff[at0]), q[tq][0]);
        }
        idct_pass<11>(d);
#pragma unroll
        for (int i = 0; i < 8; i++)
            tile[blk][i][r] = d[i];
    }
    __syncthreads();
    if (active) {
#pragma unroll
        for (int c = 0; c < 8; c++)
            d[c] = tile[blk][r][c];
        idct_pass<18>(d);
        uint2 v;
        v.x = (uint32_t)clamp255(d[0] + 128) | (uint32_t)clamp255(d[1] + 128) << 8 | (uint32_t)clamp255(d[2] + 128) << 16 |
              (uint32_t)clamp255(d[3] + 128) << 24;
        v.y = (uint32_t)clamp255(d[4] + 128) | (uint32_t)clamp255(d[5] + 128) << 8 | (uint32_t)clamp255(d[6] + 128) << 16 |
              (uint32_t)clamp255(d[7] + 128) << 24;
        uint8_t* plane = pos.comp == 0 ? a.plane[0] : pos.comp == 1 ? a.plane[1] : a.plane[2];
        *(uint2*)(plane + (size_t)(pos.y0 + r) * plane_pitch(a.g, pos.comp) + pos.x0) = v;  // (planes, pitches and x0: multiples of 8)
    }
}

// 8: four pixels of a row per lane: luma, upsampled chroma, B G R
__device__ __forceinline__ void colour_body(const Args& a, uint32_t wg)
{
    const uint32_t wq = (a.g.w + 3) / 4;
    const uint64_t idx = (uint64_t)wg * 256u + threadIdx.x;
    if (idx >= (uint64_t)wq * a.g.h)
        return;
    const uint32_t y = (uint32_t)(idx / wq), x0 = (uint32_t)(idx - (uint64_t)y * wq) * 4;
    const uint32_t n = min(4u, a.g.w - x0), py = plane_pitch(a.g, 0), pc = plane_pitch(a.g, 1);
    uint8_t px[12];
#pragma unroll
    for (uint32_t j = 0; j < 4; j++) {
        const uint32_t x = min(x0 + j, a.g.w - 1);
        const int lum = a.plane[0][(size_t)y * py + x];
        if (a.g.nc == 1) {
            if (a.out_cn == 1)
                px[j] = (uint8_t)lum;
            else
                px[3 * j] = px[3 * j + 1] = px[3 * j + 2] = (uint8_t)lum;
        } else {
            ycc_to_bgr(lum, chroma_sample(a.plane[1], pc, a.g, x, y), chroma_sample(a.plane[2], pc, a.g, x, y), px + 3 * j);
        }
    }
    uint8_t* dst = a.out + (int64_t)y * a.pitch + (int64_t)x0 * a.out_cn;
    const uint32_t nbytes = n * a.out_cn;
    if (n == 4 && ((uintptr_t)dst & 3u) == 0) {
        uint32_t* d4 = (uint32_t*)dst;
#pragma unroll
        for (uint32_t k = 0; k < 3; k++)
            if (k * 4 < nbytes)
                d4[k] = (uint32_t)px[4 * k] | (uint32_t)px[4 * k + 1] << 8 | (uint32_t)px[4 * k + 2] << 16 | (uint32_t)px[4 * k + 3] << 24;
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 12; k++)
            if (k < nbytes)
                dst[k] = px[k];
    }
}

}  // namespace jpegdec
}  // namespace v1c
