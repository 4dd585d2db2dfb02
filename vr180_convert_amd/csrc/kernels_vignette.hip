// kernels_vignette.hip -- the vignetting correction on the device: the radial gain
// pass and the ring statistics a flat-field fit starts from.  A code object of its own; the arithmetic is vignette_core.hpp's.
//   k_vig_apply  the three gain tables in LDS (6150 B); grid-stride over the items of the rows (colormatch_core.hpp: segments of 16
//                pixels read and written as 16-byte accesses, head and tail pixel by pixel), aligned on the destination; a segment is
//                read whole before it is written, so the destination may be the source
//   k_vig_zero   the ring record to zero: a graph replay starts clean, and the replay holds kernel nodes only
//   k_vig_rings  the same items; a thread merges the pixels of one ring before it adds to its WAVE's copy of the record in LDS
//                (32-bit words); every kFlushItems items the four copies of a workgroup are summed in 64 bits and leave as 64-bit
//                global atomics, zero sums left out -- vignette_core.hpp has the bound that keeps the 32-bit words from overflowing
// T is the pixels' element type (uint8_t, uint16_t), CN the channels of a pixel.  The source's 16-byte loads are unaligned wherever its
// rows start elsewhere modulo 16 than the destination's and stay 16-byte loads.
#include <hip/hip_runtime.h>

#include "vignette_launch.hpp"

namespace v1c {
namespace vignette {

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

// element j of a segment held in 32-bit words
template <class T>
__device__ __forceinline__ uint32_t elem_of(const uint32_t* w, int j)
{
    if (sizeof(T) == 1)
        return (w[j >> 2] >> (8 * (j & 3))) & 255u;
    return (w[j >> 1] >> (16 * (j & 1))) & 65535u;
}

template <class T>
struct __attribute__((packed, aligned(1))) Loose {
    T v;
};

// an element at any byte address (the C ABI asks for multiples of the element size; the form costs nothing)
template <class T>
__device__ __forceinline__ uint32_t read_elem(const uint8_t* p)
{
    return ((const Loose<T>*)p)->v;
}

template <class T>
__device__ __forceinline__ void write_elem(uint8_t* p, uint32_t v)
{
    ((Loose<T>*)p)->v = (T)v;
}

template <class T, int CN>
__global__ __launch_bounds__(kThreads) void k_vig_apply(const uint8_t* src, int64_t pitch_s, uint8_t* dst, int64_t pitch_d, int h, int w,
                                                        Geom g, const uint16_t* __restrict__ tables)
{
    constexpr int ES = sizeof(T), BPP = CN * ES, CC = CN == 1 ? 1 : 3, NW = 4 * BPP;  // NW: 32-bit words of a segment
    constexpr uint32_t kMax = ES == 1 ? 255u : 65535u;
    __shared__ uint16_t tab[kTableWords];
    for (int i = threadIdx.x; i < kTableWords; i += kThreads)
        tab[i] = tables[i];
    __syncthreads();
    const int per_row = segs_of(w) + 1;
    const int64_t items = (int64_t)h * per_row;
    for (int64_t it = (int64_t)blockIdx.x * kThreads + threadIdx.x; it < items; it += (int64_t)gridDim.x * kThreads) {
        const int y = (int)(it / per_row), s = (int)(it - (int64_t)y * per_row);
        const uint8_t* rs = src + (int64_t)y * pitch_s;
        uint8_t* rd = dst + (int64_t)y * pitch_d;
        const int64_t dy2 = sq(y - g.cy);
        const int x0 = head_of((unsigned)((uintptr_t)rd & 15u), BPP, w);
        const int nseg = (w - x0) / kSegPixels;
        if (s < per_row - 1) {
            if (s >= nseg)
                continue;
            const int xa = x0 + s * kSegPixels;
            const int64_t o = (int64_t)xa * BPP;
            uint32_t a[NW], b[NW];
#pragma unroll
            for (int k = 0; k < BPP; k++)
                load16(rs + o + 16 * k, a + 4 * k);
#pragma unroll
            for (int k = 0; k < NW; k++)
                b[k] = 0;
#pragma unroll
            for (int p = 0; p < kSegPixels; p++) {
                const Pos pos = position(dy2 + sq(xa + p - g.cx), g.scale, g.shift);
#pragma unroll
                for (int c = 0; c < CN; c++) {
                    const int j = p * CN + c;
                    uint32_t v = elem_of<T>(a, j);
                    if (c < CC)
                        v = scaled(v, gain_q14(tab + table_of<CN>(c) * (kBins + 1), pos), kMax);
                    if (ES == 1)
                        b[j >> 2] |= v << (8 * (j & 3));
                    else
                        b[j >> 1] |= v << (16 * (j & 1));
                }
            }
#pragma unroll
            for (int k = 0; k < BPP; k++)
                store16(rd + o + 16 * k, b + 4 * k);
        } else {
            const int x1 = x0 + nseg * kSegPixels;  // head [0, x0) and tail [x1, w)
            for (int x = 0; x < w; x++) {
                if (x >= x0 && x < x1) {
                    x = x1 - 1;
                    continue;
                }
                const Pos pos = position(dy2 + sq(x - g.cx), g.scale, g.shift);
                uint32_t v[CN];
#pragma unroll
                for (int c = 0; c < CN; c++)
                    v[c] = read_elem<T>(rs + ((int64_t)x * CN + c) * ES);
#pragma unroll
                for (int c = 0; c < CN; c++)
                    write_elem<T>(rd + ((int64_t)x * CN + c) * ES,
                                  c < CC ? scaled(v[c], gain_q14(tab + table_of<CN>(c) * (kBins + 1), pos), kMax) : v[c]);
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_vig_zero(unsigned long long* __restrict__ out, int words)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < words)
        out[i] = 0;
}

template <class T, int CN>
__global__ __launch_bounds__(kThreads) void k_vig_rings(const uint8_t* __restrict__ src, int64_t pitch, int h, int w, RingParams prm,
                                                        unsigned long long* __restrict__ out)
{
    constexpr int ES = sizeof(T), BPP = CN * ES, CC = CN == 1 ? 1 : 3, NW = 4 * BPP;
    extern __shared__ uint32_t copies[];  // [kWaves][rings][kRingWords]
    const int words = prm.rings * kRingWords;
    for (int i = threadIdx.x; i < kWaves * words; i += kThreads)
        copies[i] = 0;
    __syncthreads();
    uint32_t* mine = copies + (threadIdx.x >> 6) * words;
    auto add = [mine](int ring, int word, uint32_t value) { atomicAdd(&mine[ring * kRingWords + word], value); };
    RingRun run;
    const int per_row = segs_of(w) + 1;
    const int64_t items = (int64_t)h * per_row, stride = (int64_t)gridDim.x * kThreads;
    const int64_t rounds = (items + stride - 1) / stride;  // the same for every thread: the flushes below are the workgroup's
    for (int64_t r0 = 0; r0 < rounds; r0 += kFlushItems) {
        const int64_t r1 = r0 + kFlushItems < rounds ? r0 + kFlushItems : rounds;
        for (int64_t r = r0; r < r1; r++) {
            const int64_t it = r * stride + (int64_t)blockIdx.x * kThreads + threadIdx.x;
            if (it >= items)
                continue;
            const int y = (int)(it / per_row), s = (int)(it - (int64_t)y * per_row);
            const uint8_t* rs = src + (int64_t)y * pitch;
            const int64_t dy2 = sq(y - prm.cy);
            const int x0 = head_of((unsigned)((uintptr_t)rs & 15u), BPP, w);
            const int nseg = (w - x0) / kSegPixels;
            if (s < per_row - 1) {
                if (s >= nseg)
                    continue;
                const int xa = x0 + s * kSegPixels;
                uint32_t a[NW];
#pragma unroll
                for (int k = 0; k < BPP; k++)
                    load16(rs + (int64_t)xa * BPP + 16 * k, a + 4 * k);
#pragma unroll
                for (int p = 0; p < kSegPixels; p++) {
                    int v[CC];
#pragma unroll
                    for (int c = 0; c < CC; c++)
                        v[c] = (int)elem_of<T>(a, p * CN + c);
                    ring_pixel<CC>(v, dy2 + sq(xa + p - prm.cx), prm, run, add);
                }
            } else {
                const int x1 = x0 + nseg * kSegPixels;
                for (int x = 0; x < w; x++) {
                    if (x >= x0 && x < x1) {
                        x = x1 - 1;
                        continue;
                    }
                    int v[CC];
#pragma unroll
                    for (int c = 0; c < CC; c++)
                        v[c] = (int)read_elem<T>(rs + ((int64_t)x * CN + c) * ES);
                    ring_pixel<CC>(v, dy2 + sq(x - prm.cx), prm, run, add);
                }
            }
        }
        ring_flush(run, add);
        __syncthreads();
        for (int i = threadIdx.x; i < words; i += kThreads) {
            unsigned long long t = 0;
#pragma unroll
            for (int v = 0; v < kWaves; v++) {
                t += copies[v * words + i];
                copies[v * words + i] = 0;
            }
            if (t)
                atomicAdd(&out[i], t);
        }
        __syncthreads();
    }
}

int blocks_for(int h, int w)
{
    const int64_t items = (int64_t)h * (segs_of(w) + 1);
    const int64_t b = (items + kThreads - 1) / kThreads;
    return (int)(b < kMaxBlocks ? b : kMaxBlocks);
}

}  // namespace

#define V1C_VIG_DISPATCH(KERNEL, ...)                                    \
    do {                                                                 \
        if (es == 1) {                                                   \
            if (cn == 1)                                                 \
                KERNEL(uint8_t, 1, __VA_ARGS__);                         \
            else if (cn == 3)                                            \
                KERNEL(uint8_t, 3, __VA_ARGS__);                         \
            else                                                         \
                KERNEL(uint8_t, 4, __VA_ARGS__);                         \
        } else {                                                         \
            if (cn == 1)                                                 \
                KERNEL(uint16_t, 1, __VA_ARGS__);                        \
            else if (cn == 3)                                            \
                KERNEL(uint16_t, 3, __VA_ARGS__);                        \
            else                                                         \
                KERNEL(uint16_t, 4, __VA_ARGS__);                        \
        }                                                                \
    } while (0)

hipError_t launch_apply(const uint8_t* src, int64_t pitch_s, uint8_t* dst, int64_t pitch_d, int h, int w, int cn, int es, const Geom& geom,
                        const uint16_t* tables, hipStream_t st)
{
    const dim3 g(blocks_for(h, w)), b(kThreads);
#define V1C_VIG_APPLY(T, CN, ...) hipLaunchKernelGGL((k_vig_apply<T, CN>), g, b, 0, st, __VA_ARGS__)
    V1C_VIG_DISPATCH(V1C_VIG_APPLY, src, pitch_s, dst, pitch_d, h, w, geom, tables);
#undef V1C_VIG_APPLY
    return hipGetLastError();
}

hipError_t launch_rings(const uint8_t* src, int64_t pitch, int h, int w, int cn, int es, const RingParams& prm, int64_t* rings, hipStream_t st)
{
    const int words = prm.rings * kRingWords;
    unsigned long long* out = (unsigned long long*)rings;
    hipLaunchKernelGGL(k_vig_zero, dim3((words + kThreads - 1) / kThreads), dim3(kThreads), 0, st, out, words);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    const dim3 g(blocks_for(h, w)), b(kThreads);
    const size_t lds = (size_t)kWaves * words * sizeof(uint32_t);  // 1 KiB (16 rings) .. 64 KiB (1024)
#define V1C_VIG_RINGS(T, CN, ...) hipLaunchKernelGGL((k_vig_rings<T, CN>), g, b, lds, st, __VA_ARGS__)
    V1C_VIG_DISPATCH(V1C_VIG_RINGS, src, pitch, h, w, prm, out);
#undef V1C_VIG_RINGS
    return hipGetLastError();
}

}  // namespace vignette
}  // namespace v1c
