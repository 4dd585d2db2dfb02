// colormatch_core.hpp -- the arithmetic of the colour match of the two eyes (v1c_color_match_luts_async / v1c_apply_luts_async,
// INTEGRATION.md section 12; tests/colormatch_ref.py restates it), shared by the kernels (kernels_colormatch.hip) and by the host
// emulation (tests/host_colormatch/colormatch_emul.hip): the joint mask, the merge of equal neighbours in front of the histogram add,
// one bin's entry of either table and the report record.  Integer arithmetic throughout.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define V1C_CM_HD __host__ __device__ inline
#else
#define V1C_CM_HD inline
#endif

namespace v1c {
namespace colormatch {

constexpr int kBins = 256;
constexpr int kHistWords = 2 * 3 * kBins;   // h[eye][channel][bin], eye 0 = left: the workspace, and one wave's copy in LDS (6 KiB)
constexpr int kLutBytes = 3 * kBins;
constexpr int kReportWords = 20;            // status, n, per channel (first, last of the left eye, of the right eye, g), two spare
constexpr int kModeHistogram = 0, kModeGain = 1;
constexpr int64_t kGainMin = 16384, kGainMax = 262144;  // 1/4 .. 4 in 1/65536

// what v1c_color_match_params resolves to (include/vr180_remap.h)
struct Params {
    int32_t mode, reference, lo, hi, max_shift, min_pixels;
};

V1C_CM_HD bool counted(int max_left, int max_right, int lo, int hi)
{
    return (max_left >= lo) & (max_left <= hi) & (max_right >= lo) & (max_right <= hi);
}

// ---- the merge in front of the histogram add: a thread walks its pixels in order and keeps, per eye and channel, the value it saw
// last and how often in a row; the add goes out when the value changes and at the end.  A flat frame costs one add per thread and
// slot, not one per pixel.
struct RunSlot {
    int value = -1;
    uint32_t count = 0;
};

// add(slot, bin, count) receives what leaves a slot; slot = 3 * eye + channel
template <class Add>
V1C_CM_HD void run_step(RunSlot& s, int slot, int v, Add& add)
{
    if (v == s.value) {
        s.count++;
        return;
    }
    if (s.count)
        add(slot, s.value, s.count);
    s.value = v;
    s.count = 1;
}

// one position of both eyes: l, r hold the CC colour channels' values; rs: the thread's six slots
template <int CC, class Add>
V1C_CM_HD void count_pixel(const int* l, const int* r, int lo, int hi, RunSlot* rs, Add& add)
{
    int ml = l[0], mr = r[0];
    if (CC == 3) {
        ml = l[1] > ml ? l[1] : ml;
        ml = l[2] > ml ? l[2] : ml;
        mr = r[1] > mr ? r[1] : mr;
        mr = r[2] > mr ? r[2] : mr;
    }
    if (!counted(ml, mr, lo, hi))
        return;
#pragma unroll
    for (int c = 0; c < CC; c++) {
        run_step(rs[c], c, l[c], add);
        run_step(rs[3 + c], 3 + c, r[c], add);
    }
}

template <class Add>
V1C_CM_HD void run_flush(RunSlot* rs, Add& add)
{
#pragma unroll
    for (int k = 0; k < 6; k++)
        if (rs[k].count)
            add(k, rs[k].value, rs[k].count);
}

// ---- a row as work items: the pixels in front of the first one whose byte address is a multiple of 16 (the head), segments of 16
// pixels from there -- 16 * cn bytes, cn loads of 16 bytes --, and what is left (the tail).  Item segs_of(w) of a row is its head and
// tail together, walked pixel by pixel; items below it are its segments, and those past the row's last whole segment are empty.
constexpr int kSegPixels = 16;
V1C_CM_HD int segs_of(int w) { return w / kSegPixels; }

// the head of a row that starts at an address with these low four bits: the smallest x < 16 with (a + x cn) % 16 == 0, 0 where there
// is none (cn 4 on an address that is no multiple of 4: every load of that row is unaligned), never more than w
V1C_CM_HD int head_of(unsigned a, int cn, int w)
{
    int x = 0;
    for (int k = 0; k < kSegPixels; k++)
        if (((a + (unsigned)(k * cn)) & 15u) == 0) {
            x = k;
            break;
        }
    return x < w ? x : w;
}

// ---- mode "histogram".  CT / CR: the running (inclusive) sums of the target's and the reference's counts of one channel, knots: bit v
// of the 256-bit mask is set where bin v is a knot (the target's bin v is populated, or v is 0 or 255)
V1C_CM_HD int knot_value(const uint32_t* CT, const uint32_t* CR, int v)
{
    const uint32_t below = v ? CT[v - 1] : 0;
    if (CT[v] == below)
        return v;  // (0, 0) or (255, 255)
    const uint64_t mid2 = (uint64_t)below + CT[v];
    int lo = 0, hi = kBins - 1;  // min u with 2 CR[u] >= mid2; CR[255] = CT[255] >= mid2 / 2
    while (lo < hi) {
        const int u = (lo + hi) >> 1;
        if (2 * (uint64_t)CR[u] >= mid2)
            hi = u;
        else
            lo = u + 1;
    }
    return lo;
}

V1C_CM_HD int high_bit64(uint64_t v)  // v != 0
{
#if defined(__HIP_DEVICE_COMPILE__)
    return 63 - __clzll((long long)v);
#else
    return 63 - __builtin_clzll(v);
#endif
}

V1C_CM_HD int low_bit64(uint64_t v)  // v != 0
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __ffsll((unsigned long long)v) - 1;
#else
    return __builtin_ctzll(v);
#endif
}

// the nearest knot below v (bit 0 is always set), 0 < v
V1C_CM_HD int knot_below(const uint64_t* knots, int v)
{
    int w = (v - 1) >> 6;
    uint64_t m = knots[w] & (~0ull >> (63 - ((v - 1) & 63)));
    while (!m)
        m = knots[--w];
    return 64 * w + high_bit64(m);
}

// the nearest knot above v (bit 255 is always set), v < 255
V1C_CM_HD int knot_above(const uint64_t* knots, int v)
{
    int w = (v + 1) >> 6;
    uint64_t m = knots[w] & (~0ull << ((v + 1) & 63));
    while (!m)
        m = knots[++w];
    return 64 * w + low_bit64(m);
}

V1C_CM_HD int clamp_shift(int m, int v, int max_shift)
{
    m = m < v - max_shift ? v - max_shift : m;
    m = m > v + max_shift ? v + max_shift : m;
    return m < 0 ? 0 : m > 255 ? 255 : m;
}

V1C_CM_HD uint8_t histogram_entry(const uint32_t* CT, const uint32_t* CR, const uint64_t* knots, int v, int max_shift)
{
    int m;
    if ((knots[v >> 6] >> (v & 63)) & 1) {
        m = knot_value(CT, CR, v);
    } else {
        const int a = knot_below(knots, v), b = knot_above(knots, v);
        const int ma = knot_value(CT, CR, a), mb = knot_value(CT, CR, b);
        m = ma + ((v - a) * (mb - ma) * 2 + (b - a)) / (2 * (b - a));  // (mb >= ma: no negative dividend)
    }
    return (uint8_t)clamp_shift(m, v, max_shift);
}

// ---- mode "gain".  sT > 0; sums are below 255 * 2^31, so sR * 65536 stays within int64
V1C_CM_HD int64_t gain_of(int64_t sT, int64_t sR)
{
    const int64_t g = (sR * 65536 + sT / 2) / sT;
    return g < kGainMin ? kGainMin : g > kGainMax ? kGainMax : g;
}

V1C_CM_HD uint8_t gain_entry(int v, int64_t g)
{
    const int64_t m = ((int64_t)v * g + 32768) >> 16;
    return (uint8_t)(m > 255 ? 255 : m);
}

}  // namespace colormatch
}  // namespace v1c
