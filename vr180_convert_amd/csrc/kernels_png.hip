// kernels_png.hip -- the device PNG encoder's kernels: filter, distance-1 run tokens, histograms and Adler-32 partials (pass 1); bit
// counts, the scan over a band's segments, bit packing, stored bands and the host's words (pass 2).  INTEGRATION.md section 6 has the
// stream contract, DESIGN.md section 12 the design.  A code object of its own: the remap kernels do not change with it.
//
// One wave takes one 256-byte segment of a band's scanlines at a time, one byte per lane in four steps; a workgroup of four waves walks
// kSegsPerGroup consecutive segments of one band.  Every lane does a bounded amount of work and nothing waits on another workgroup.
// Words of the stream that two segments share are written with atomic ORs of disjoint bits into a zeroed buffer, words a segment owns
// with plain stores: the result does not depend on any order.
#include <hip/hip_runtime.h>

#include "png_launch.hpp"

namespace v1c {
namespace png {

namespace {

struct BandGeom {
    uint32_t row0, nbytes, nseg;
};

__device__ inline BandGeom band_geom(const Args& a, uint32_t band)
{
    BandGeom g;
    g.row0 = band * a.band_rows;
    const uint32_t rows = min(a.band_rows, a.h - g.row0);
    g.nbytes = rows * a.stride;
    g.nseg = (g.nbytes + kSeg - 1) / kSeg;
    return g;
}

constexpr uint32_t kNoByte = 0x200;  // a lane past the band's end: equal to no byte

// the wave's segment: v[c] = filtered byte 64 * c + lane (kNoByte past the end), eq = the 256-bit "equals the byte before" mask
template <int BPP>
__device__ inline void load_segment(const Args& a, const BandGeom& g, uint32_t seg, int lane, uint32_t v[4], uint64_t eq[4])
{
    uint32_t carry = 0x100;  // the segment's first byte repeats nothing
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const uint32_t q = seg * kSeg + c * 64 + lane;
        uint32_t b = kNoByte;
        if (q < g.nbytes) {
            const uint32_t r = q / a.stride;
            b = filtered_byte(a.img, a.pitch, BPP, a.filter, g.row0 + r, q - r * a.stride);
        }
        uint32_t prev = __shfl_up(b, 1);
        prev = lane ? prev : carry;
        eq[c] = __ballot(b == prev && b != kNoByte);
        carry = __shfl(b, 63);
        v[c] = b;
    }
}

__device__ inline uint32_t wave_sum(uint32_t x)
{
#pragma unroll
    for (int d = 32; d; d >>= 1)
        x += __shfl_xor(x, d);
    return x;
}

__device__ inline unsigned long long wave_sum64(unsigned long long x)
{
#pragma unroll
    for (int d = 32; d; d >>= 1)
        x += __shfl_xor(x, d);
    return x;
}

__device__ inline uint32_t wave_inclusive_scan(uint32_t x, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d);
        x += lane >= d ? y : 0;
    }
    return x;
}

}  // namespace

// pass 1: the band's symbol counts and the two sums of its Adler-32
template <int BPP>
__global__ __launch_bounds__(256) void k_png_hist(Args a)
{
    __shared__ uint32_t h[kHistStride];
    const uint32_t band = blockIdx.x / a.groups, grp = blockIdx.x % a.groups;
    const BandGeom g = band_geom(a, band);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int i = tid; i < kHistStride; i += 256)
        h[i] = 0;
    __syncthreads();
    unsigned long long s1 = 0, s2 = 0;
    for (int it = 0; it < kSegsPerGroup / 4; it++) {
        const uint32_t seg = grp * kSegsPerGroup + it * 4 + wave;
        if (seg >= g.nseg)
            break;
        uint32_t v[4];
        uint64_t eq[4];
        load_segment<BPP>(a, g, seg, lane, v, eq);
#pragma unroll
        for (int c = 0; c < 4; c++) {
            if (v[c] == kNoByte)
                continue;
            int length;
            const int kind = classify(eq, c, lane, &length);
            if (kind != kNone)
                atomicAdd(&h[token_symbol(kind, v[c], length)], 1u);
            const uint32_t q = seg * kSeg + c * 64 + lane;
            s1 += v[c];
            s2 += (unsigned long long)(g.nbytes - q) * v[c];
        }
    }
    s1 = wave_sum64(s1);
    s2 = wave_sum64(s2);
    if (lane == 0 && s1) {
        atomicAdd(&a.adler[2 * band], s1);
        atomicAdd(&a.adler[2 * band + 1], s2 % kAdlerBase);
    }
    __syncthreads();
    for (int i = tid; i < kSymbols; i += 256)
        if (h[i])
            atomicAdd(&a.hist[(size_t)band * kHistStride + i], h[i]);
}

// pass 2a: the bits every segment's tokens take with the band's code
template <int BPP>
__global__ __launch_bounds__(256) void k_png_bits(Args a)
{
    __shared__ uint32_t table[kSymbols];
    const uint32_t band = blockIdx.x / a.groups, grp = blockIdx.x % a.groups;
    if (a.bands[band].stored)
        return;
    const BandGeom g = band_geom(a, band);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int i = tid; i < kSymbols; i += 256)
        table[i] = a.tables[(size_t)band * kSymbols + i];
    __syncthreads();
    for (int it = 0; it < kSegsPerGroup / 4; it++) {
        const uint32_t seg = grp * kSegsPerGroup + it * 4 + wave;
        if (seg >= g.nseg)
            break;
        uint32_t v[4];
        uint64_t eq[4];
        load_segment<BPP>(a, g, seg, lane, v, eq);
        uint32_t bits = 0;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            int length = 0, nb;
            const int kind = v[c] == kNoByte ? (int)kNone : classify(eq, c, lane, &length);
            (void)token_bits(table, kind, v[c] & 255u, length, &nb);
            bits += (uint32_t)nb;
        }
        bits = wave_sum(bits);
        if (lane == 0)
            a.segbits[(size_t)band * a.segs_per_band + seg] = bits;
    }
}

// pass 2b: exclusive scan of a band's segment sizes; one workgroup per band
__global__ __launch_bounds__(256) void k_png_scan(Args a)
{
    __shared__ unsigned long long tmp[256];
    const uint32_t band = blockIdx.x;
    if (a.bands[band].stored)
        return;
    const BandGeom g = band_geom(a, band);
    const int tid = threadIdx.x;
    unsigned long long carry = a.bands[band].token_bit0;
    for (uint32_t i0 = 0; i0 < g.nseg; i0 += 256) {
        const uint32_t i = i0 + tid;
        const unsigned long long v = i < g.nseg ? a.segbits[(size_t)band * a.segs_per_band + i] : 0;
        unsigned long long x = v;
        tmp[tid] = x;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const unsigned long long y = tid >= d ? tmp[tid - d] : 0;
            __syncthreads();
            x += y;
            tmp[tid] = x;
            __syncthreads();
        }
        if (i < g.nseg)
            a.segoff[(size_t)band * a.segs_per_band + i] = carry + x - v;
        carry += tmp[255];
        __syncthreads();
    }
}

// pass 2c: every segment's tokens at the segment's bit offset: assembled in LDS, stored as whole words
template <int BPP>
__global__ __launch_bounds__(256) void k_png_pack(Args a)
{
    __shared__ uint32_t table[kSymbols];
    __shared__ uint32_t buf[4][128];  // a segment is at most 256 * 15 bits behind up to 31 bits of its first word: 121 words
    const uint32_t band = blockIdx.x / a.groups, grp = blockIdx.x % a.groups;
    if (a.bands[band].stored)
        return;
    const BandGeom g = band_geom(a, band);
    if (grp * kSegsPerGroup >= g.nseg)
        return;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int i = tid; i < kSymbols; i += 256)
        table[i] = a.tables[(size_t)band * kSymbols + i];
    for (int it = 0; it < kSegsPerGroup / 4; it++) {  // (the same trip count for all four waves: the barriers are uniform)
        const uint32_t seg = grp * kSegsPerGroup + it * 4 + wave;
        const bool active = seg < g.nseg;
        buf[wave][lane] = 0;
        buf[wave][lane + 64] = 0;
        __syncthreads();
        unsigned long long start = 0;
        uint32_t end = 0;  // bits of the segment behind bit 0 of its first word
        if (active) {
            uint32_t v[4];
            uint64_t eq[4];
            load_segment<BPP>(a, g, seg, lane, v, eq);
            start = a.segoff[(size_t)band * a.segs_per_band + seg];
            end = (uint32_t)(start & 31);
#pragma unroll
            for (int c = 0; c < 4; c++) {
                int length = 0, nb;
                const int kind = v[c] == kNoByte ? (int)kNone : classify(eq, c, lane, &length);
                const uint32_t bits = token_bits(table, kind, v[c] & 255u, length, &nb);
                const uint32_t incl = wave_inclusive_scan((uint32_t)nb, lane);
                if (nb) {
                    const uint32_t pos = end + incl - (uint32_t)nb;
                    const unsigned long long x = (unsigned long long)bits << (pos & 31);
                    atomicOr(&buf[wave][pos >> 5], (uint32_t)x);
                    if (x >> 32)
                        atomicOr(&buf[wave][(pos >> 5) + 1], (uint32_t)(x >> 32));
                }
                end += __shfl(incl, 63);
            }
        }
        __syncthreads();
        if (active) {
            const uint32_t nwords = (end + 31) >> 5;
            uint32_t* dst = a.out + (start >> 5);
#pragma unroll
            for (int k0 = 0; k0 < 128; k0 += 64) {
                const uint32_t k = k0 + lane;
                if (k < nwords) {
                    const uint32_t w = buf[wave][k];
                    if (k == 0 || k == nwords - 1) {  // possibly shared with a neighbour, the header or the band's tail
                        if (w)
                            atomicOr(&dst[k], w);
                    } else {
                        dst[k] = w;
                    }
                }
            }
        }
        __syncthreads();
    }
}

// pass 2d: the data bytes of the bands that go out as stored blocks
template <int BPP>
__global__ __launch_bounds__(256) void k_png_store(Args a)
{
    const uint32_t band = blockIdx.x / a.groups, grp = blockIdx.x % a.groups;
    if (!a.bands[band].stored)
        return;
    const BandGeom g = band_geom(a, band);
    uint8_t* dst = (uint8_t*)a.out + a.bands[band].byte0;
    for (int it = 0; it < kSegsPerGroup; it++) {
        const uint32_t q = (grp * kSegsPerGroup + it) * kSeg + threadIdx.x;
        if (q >= g.nbytes)
            break;
        const uint32_t r = q / a.stride;
        dst[stored_position(q)] = (uint8_t)filtered_byte(a.img, a.pitch, BPP, a.filter, g.row0 + r, q - r * a.stride);
    }
}

// pass 2e: the host's words (block headers, end-of-block codes, stored-block headers); runs after the kernels above
__global__ __launch_bounds__(256) void k_png_or(const OrWord* list, uint32_t n, uint32_t* out)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i < n)
        atomicOr(&out[list[i].word], list[i].value);
}

#define PNG_FOR_BPP(K, grid, ...)                                                    \
    switch (bpp) {                                                                   \
    case 1: hipLaunchKernelGGL(K<1>, grid, dim3(256), 0, st, __VA_ARGS__); break;    \
    case 2: hipLaunchKernelGGL(K<2>, grid, dim3(256), 0, st, __VA_ARGS__); break;    \
    case 3: hipLaunchKernelGGL(K<3>, grid, dim3(256), 0, st, __VA_ARGS__); break;    \
    case 4: hipLaunchKernelGGL(K<4>, grid, dim3(256), 0, st, __VA_ARGS__); break;    \
    case 6: hipLaunchKernelGGL(K<6>, grid, dim3(256), 0, st, __VA_ARGS__); break;    \
    case 8: hipLaunchKernelGGL(K<8>, grid, dim3(256), 0, st, __VA_ARGS__); break;    \
    default: return hipErrorInvalidValue;                                            \
    }

hipError_t launch_pass1(const Args& a, int bpp, hipStream_t st)
{
    const dim3 grid(a.n_bands * a.groups);
    PNG_FOR_BPP(k_png_hist, grid, a)
    return hipGetLastError();
}

hipError_t launch_pass2(const Args& a, int bpp, bool any_coded, bool any_stored, const OrWord* list, uint32_t n_or, hipStream_t st)
{
    const dim3 grid(a.n_bands * a.groups);
    if (any_coded) {
        PNG_FOR_BPP(k_png_bits, grid, a)
        hipLaunchKernelGGL(k_png_scan, dim3(a.n_bands), dim3(256), 0, st, a);
        PNG_FOR_BPP(k_png_pack, grid, a)
    }
    if (any_stored) {
        PNG_FOR_BPP(k_png_store, grid, a)
    }
    if (n_or)
        hipLaunchKernelGGL(k_png_or, dim3((n_or + 255) / 256), dim3(256), 0, st, list, n_or, a.out);
    return hipGetLastError();
}

}  // namespace png
}  // namespace v1c
