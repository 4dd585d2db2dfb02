// kernels_colormatch.hip -- the colour match of the two eyes on the device: joint-mask
// histograms of both eyes, the three 256-entry tables, and the rewrite of the target eye through them.  A code object of its own; the
// arithmetic is colormatch_core.hpp's.
//   k_cm_zero   the workspace's 1536 counters to zero
//   k_cm_hist   grid-stride over the items of both eyes' rows (colormatch_core.hpp: segments of 16 pixels read as 16-byte loads, head and
//               tail pixel by pixel); a thread merges equal values that follow each other before it adds to its WAVE's copy of the
//               histograms in LDS; the four copies of a workgroup are summed and leave as integer global atomics, zero sums left out
//   k_cm_luts   one workgroup, one thread per bin: running sums by a scan in LDS, populated-bin masks by ballot, the knots and the
//               interpolation or the gain, the tables and the report record
//   k_cm_apply  the tables in LDS (768 B), the same items, aligned on the destination: 16-byte loads and stores
// A row's head is chosen on the LEFT eye's (the destination's) address; the other image's 16-byte loads are unaligned wherever its rows
// start elsewhere modulo 16 -- the right half of an odd-width side-by-side frame always -- and stay 16-byte loads.
#include <hip/hip_runtime.h>

#include "colormatch_launch.hpp"

namespace v1c {
namespace colormatch {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxBlocks = 1024;  // four workgroups per CU: 16 waves with 16-byte loads in flight

struct __attribute__((packed, aligned(1))) Bytes16 {
    uint32_t w[4];
};

__device__ __forceinline__ void load16(const uint8_t* p, uint32_t* w)
{
    const Bytes16 v = *(const Bytes16*)p;
#pragma unroll
    for (int k = 0; k < 4; k++)
        w[k] = v.w[k];
}

__device__ __forceinline__ void store16(uint8_t* p, const uint32_t* w)
{
    Bytes16 v;
#pragma unroll
    for (int k = 0; k < 4; k++)
        v.w[k] = w[k];
    *(Bytes16*)p = v;
}

__device__ __forceinline__ int byte_of(const uint32_t* w, int j) { return (int)((w[j >> 2] >> (8 * (j & 3))) & 255u); }

// the workspace's counters, zeroed by a launch of the chain's own: a graph replay starts clean, and the replay holds kernel nodes only
__global__ __launch_bounds__(kThreads) void k_cm_zero(uint32_t* __restrict__ hist)
{
    hist[blockIdx.x * kThreads + threadIdx.x] = 0;
}

template <int CN>
__global__ __launch_bounds__(kThreads) void k_cm_hist(const uint8_t* __restrict__ left, int64_t pitch_l, const uint8_t* __restrict__ right,
                                                      int64_t pitch_r, int h, int w, int lo, int hi, uint32_t* __restrict__ hist)
{
    constexpr int CC = CN == 1 ? 1 : 3;
    __shared__ uint32_t copies[kWaves][kHistWords];
    for (int i = threadIdx.x; i < kWaves * kHistWords; i += kThreads)
        (&copies[0][0])[i] = 0;
    __syncthreads();
    uint32_t* mine = copies[threadIdx.x >> 6];
    auto add = [mine](int slot, int bin, uint32_t count) { atomicAdd(&mine[slot * kBins + bin], count); };
    RunSlot rs[6];
    const int per_row = segs_of(w) + 1;
    const int64_t items = (int64_t)h * per_row;
    for (int64_t it = (int64_t)blockIdx.x * kThreads + threadIdx.x; it < items; it += (int64_t)gridDim.x * kThreads) {
        const int y = (int)(it / per_row), s = (int)(it - (int64_t)y * per_row);
        const uint8_t* rl = left + (int64_t)y * pitch_l;
        const uint8_t* rr = right + (int64_t)y * pitch_r;
        const int x0 = head_of((unsigned)((uintptr_t)rl & 15u), CN, w);
        const int nseg = (w - x0) / kSegPixels;
        if (s < per_row - 1) {
            if (s >= nseg)
                continue;
            const int64_t o = (int64_t)(x0 + s * kSegPixels) * CN;
            uint32_t a[4 * CN], b[4 * CN];
#pragma unroll
            for (int k = 0; k < CN; k++) {
                load16(rl + o + 16 * k, a + 4 * k);
                load16(rr + o + 16 * k, b + 4 * k);
            }
#pragma unroll
            for (int p = 0; p < kSegPixels; p++) {
                int l[3], r[3];
#pragma unroll
                for (int c = 0; c < CC; c++) {
                    l[c] = byte_of(a, p * CN + c);
                    r[c] = byte_of(b, p * CN + c);
                }
                count_pixel<CC>(l, r, lo, hi, rs, add);
            }
        } else {
            const int x1 = x0 + nseg * kSegPixels;  // head [0, x0) and tail [x1, w)
            for (int x = 0; x < w; x++) {
                if (x >= x0 && x < x1) {
                    x = x1 - 1;
                    continue;
                }
                int l[3], r[3];
#pragma unroll
                for (int c = 0; c < CC; c++) {
                    l[c] = rl[(int64_t)x * CN + c];
                    r[c] = rr[(int64_t)x * CN + c];
                }
                count_pixel<CC>(l, r, lo, hi, rs, add);
            }
        }
    }
    run_flush(rs, add);
    __syncthreads();
    for (int i = threadIdx.x; i < kHistWords; i += kThreads) {
        uint32_t t = 0;
#pragma unroll
        for (int v = 0; v < kWaves; v++)
            t += copies[v][i];
        if (t)
            atomicAdd(&hist[i], t);
    }
}

__device__ __forceinline__ int64_t wave_sum64(int64_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        v += __shfl_xor((long long)v, o, 64);
    return v;
}

__global__ __launch_bounds__(kBins) void k_cm_luts(const uint32_t* __restrict__ hist, int cc, Params prm, uint8_t* __restrict__ luts,
                                                   int32_t* __restrict__ report)
{
    __shared__ uint32_t cum[2][3][kBins];     // counts, then their running sums
    __shared__ uint64_t pop[2][3][kWaves];    // populated bins
    __shared__ int64_t wsum[2][3][kWaves];    // sum of v * count, per wave
    __shared__ uint64_t knots[3][kWaves];     // the target's populated bins and bins 0 and 255
    const int v = threadIdx.x, wave = v >> 6;
    int64_t part[2][3];
#pragma unroll
    for (int e = 0; e < 2; e++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const uint32_t t = hist[(e * 3 + c) * kBins + v];
            cum[e][c][v] = t;
            const uint64_t m = __ballot(t != 0);
            part[e][c] = wave_sum64((int64_t)v * t);
            if ((v & 63) == 0) {
                pop[e][c][wave] = m;
                wsum[e][c][wave] = part[e][c];
            }
        }
    __syncthreads();
    if (v < 3 * kWaves) {
        const int k = v & (kWaves - 1);
        knots[v / kWaves][k] = pop[1 - prm.reference][v / kWaves][k] | (k == 0 ? 1ull : 0ull) | (k == kWaves - 1 ? 1ull << 63 : 0ull);
    }
    for (int o = 1; o < kBins; o <<= 1) {
        uint32_t t[6];
#pragma unroll
        for (int k = 0; k < 6; k++)
            t[k] = v >= o ? (&cum[0][0][0])[k * kBins + v - o] : 0;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 6; k++)
            (&cum[0][0][0])[k * kBins + v] += t[k];
        __syncthreads();
    }
    const int ref = prm.reference, tgt = 1 - ref;
    const int64_t n = cum[0][0][kBins - 1];
    int64_t g[3] = {0, 0, 0};
    int status = n < prm.min_pixels ? 1 : 0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        if (c < cc && prm.mode == kModeGain) {
            int64_t sT = 0, sR = 0;
#pragma unroll
            for (int k = 0; k < kWaves; k++) {
                sT += wsum[tgt][c][k];
                sR += wsum[ref][c][k];
            }
            if (sT == 0)
                status = status ? status : 2;
            else
                g[c] = gain_of(sT, sR);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        uint8_t m = (uint8_t)v;
        if (c < cc && status == 0) {
            if (prm.mode == kModeGain) {
                m = gain_entry(v, g[c]);
            } else {
                m = histogram_entry(cum[tgt][c], cum[ref][c], knots[c], v, prm.max_shift);
            }
        }
        luts[c * kBins + v] = m;
    }
    if (v < kReportWords) {
        int32_t r = 0;
        if (v == 0)
            r = status;
        else if (v == 1)
            r = (int32_t)n;
        else if (v < 17) {
            const int c = (v - 2) / 5, k = (v - 2) % 5;
            if (k == 4) {
                r = (int32_t)(c == 0 ? g[0] : c == 1 ? g[1] : g[2]);
            } else {
                const uint64_t* m = pop[k >> 1][c];
                r = -1;
                if (c < cc && (m[0] | m[1] | m[2] | m[3])) {
                    if (k & 1) {
                        int q = kWaves - 1;
                        while (!m[q])
                            q--;
                        r = 64 * q + high_bit64(m[q]);
                    } else {
                        int q = 0;
                        while (!m[q])
                            q++;
                        r = 64 * q + low_bit64(m[q]);
                    }
                }
            }
        }
        report[v] = r;
    }
}

template <int CN>
__global__ __launch_bounds__(kThreads) void k_cm_apply(const uint8_t* src, int64_t pitch_s, uint8_t* dst, int64_t pitch_d, int h, int w,
                                                       const uint8_t* __restrict__ luts)
{
    constexpr int CC = CN == 1 ? 1 : 3;
    __shared__ uint8_t lut[kLutBytes];
    for (int i = threadIdx.x; i < kLutBytes; i += kThreads)
        lut[i] = luts[i];
    __syncthreads();
    const int per_row = segs_of(w) + 1;
    const int64_t items = (int64_t)h * per_row;
    for (int64_t it = (int64_t)blockIdx.x * kThreads + threadIdx.x; it < items; it += (int64_t)gridDim.x * kThreads) {
        const int y = (int)(it / per_row), s = (int)(it - (int64_t)y * per_row);
        const uint8_t* rs = src + (int64_t)y * pitch_s;
        uint8_t* rd = dst + (int64_t)y * pitch_d;
        const int x0 = head_of((unsigned)((uintptr_t)rd & 15u), CN, w);
        const int nseg = (w - x0) / kSegPixels;
        if (s < per_row - 1) {
            if (s >= nseg)
                continue;
            const int64_t o = (int64_t)(x0 + s * kSegPixels) * CN;
            uint32_t a[4 * CN], b[4 * CN];
#pragma unroll
            for (int k = 0; k < CN; k++)
                load16(rs + o + 16 * k, a + 4 * k);
#pragma unroll
            for (int k = 0; k < 4 * CN; k++) {
                uint32_t t = 0;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int j = 4 * k + q, c = j % CN;
                    const uint32_t val = (uint32_t)byte_of(a, j);
                    t |= (c < CC ? (uint32_t)lut[c * kBins + val] : val) << (8 * q);
                }
                b[k] = t;
            }
#pragma unroll
            for (int k = 0; k < CN; k++)
                store16(rd + o + 16 * k, b + 4 * k);
        } else {
            const int x1 = x0 + nseg * kSegPixels;
            for (int x = 0; x < w; x++) {
                if (x >= x0 && x < x1) {
                    x = x1 - 1;
                    continue;
                }
#pragma unroll
                for (int c = 0; c < CN; c++) {
                    const uint8_t val = rs[(int64_t)x * CN + c];
                    rd[(int64_t)x * CN + c] = c < CC ? lut[c * kBins + val] : val;
                }
            }
        }
    }
}

int blocks_for(int h, int w)
{
    const int64_t items = (int64_t)h * (segs_of(w) + 1);
    const int64_t b = (items + kThreads - 1) / kThreads;
    return (int)(b < kMaxBlocks ? b : kMaxBlocks);
}

}  // namespace

hipError_t launch_luts(const uint8_t* left, int64_t pitch_l, const uint8_t* right, int64_t pitch_r, int h, int w, int cn, const Params& prm,
                       uint32_t* workspace, uint8_t* luts, int32_t* report, hipStream_t st)
{
    static_assert(kHistWords % kThreads == 0, "k_cm_zero writes whole workgroups");
    hipLaunchKernelGGL(k_cm_zero, dim3(kHistWords / kThreads), dim3(kThreads), 0, st, workspace);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    const dim3 g(blocks_for(h, w)), b(kThreads);
    if (cn == 1)
        hipLaunchKernelGGL(k_cm_hist<1>, g, b, 0, st, left, pitch_l, right, pitch_r, h, w, prm.lo, prm.hi, workspace);
    else if (cn == 3)
        hipLaunchKernelGGL(k_cm_hist<3>, g, b, 0, st, left, pitch_l, right, pitch_r, h, w, prm.lo, prm.hi, workspace);
    else
        hipLaunchKernelGGL(k_cm_hist<4>, g, b, 0, st, left, pitch_l, right, pitch_r, h, w, prm.lo, prm.hi, workspace);
    e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_cm_luts, dim3(1), dim3(kBins), 0, st, (const uint32_t*)workspace, cn == 1 ? 1 : 3, prm, luts, report);
    return hipGetLastError();
}

hipError_t launch_apply(const uint8_t* src, int64_t pitch_s, uint8_t* dst, int64_t pitch_d, int h, int w, int cn, const uint8_t* luts,
                        hipStream_t st)
{
    const dim3 g(blocks_for(h, w)), b(kThreads);
    if (cn == 1)
        hipLaunchKernelGGL(k_cm_apply<1>, g, b, 0, st, src, pitch_s, dst, pitch_d, h, w, luts);
    else if (cn == 3)
        hipLaunchKernelGGL(k_cm_apply<3>, g, b, 0, st, src, pitch_s, dst, pitch_d, h, w, luts);
    else
        hipLaunchKernelGGL(k_cm_apply<4>, g, b, 0, st, src, pitch_s, dst, pitch_d, h, w, luts);
    return hipGetLastError();
}

}  // namespace colormatch
}  // namespace v1c
