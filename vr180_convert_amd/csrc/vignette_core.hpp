// vignette_core.hpp -- the arithmetic of the vignetting correction (v1c_vignette_apply_async / v1c_vignette_rings_async, INTEGRATION.md
// section 14; tests/vignette_ref.py restates it), shared by the kernels (kernels_vignette.hip) and by the host emulation
// (tests/host_vignette/vignette_emul.hip): the squared distance, the table position, the interpolated Q14 gain and the rounded product;
// the ring of a pixel and the merge of equal rings in front of the accumulator add.  Integer arithmetic throughout.  The rows are
// walked as colormatch_core.hpp's items (head, 16-pixel segments, tail), with a pixel's bytes in place of its channels.
#pragma once

#include <stdint.h>

#include "colormatch_core.hpp"

namespace v1c {
namespace vignette {

using colormatch::head_of;
using colormatch::kSegPixels;
using colormatch::segs_of;

constexpr int kBins = 1024;                    // intervals of a table
constexpr int kTableWords = 3 * (kBins + 1);   // T[channel][0 .. kBins], BGR, uint16 in Q14: 6150 B in LDS
constexpr int kScaleBits = 30, kR2Bits = 34;   // scale < 2^30 and r2 < 2^34: r2 * scale stays below 2^64
constexpr int kRingsMin = 16, kRingsMax = 1024;
constexpr int kRingWords = 4;                  // sumB, sumG, sumR, n

// what v1c_vignette_geom resolves to
struct Geom {
    int32_t cx, cy;
    uint32_t scale;
    int32_t shift;
};

// what v1c_vignette_ring_params resolves to
struct RingParams {
    int32_t cx, cy;
    int64_t r2;
    int32_t rings, lo, hi;
};

V1C_CM_HD int64_t sq(int d) { return (int64_t)d * d; }

// the largest r2 of an h x w frame around (cx, cy): one of the corners
V1C_CM_HD int64_t max_r2(int h, int w, int cx, int cy)
{
    const int64_t x0 = cx < 0 ? -(int64_t)cx : cx, x1 = (int64_t)w - 1 - cx < 0 ? (int64_t)cx - (w - 1) : (int64_t)w - 1 - cx;
    const int64_t y0 = cy < 0 ? -(int64_t)cy : cy, y1 = (int64_t)h - 1 - cy < 0 ? (int64_t)cy - (h - 1) : (int64_t)h - 1 - cy;
    const int64_t dx = x0 > x1 ? x0 : x1, dy = y0 > y1 ? y0 : y1;
    return dx * dx + dy * dy;
}

// ---- the gain pass.  The table position of a pixel: idx and the 8-bit fraction f, the last interval held beyond the table
struct Pos {
    uint32_t idx, f;
};

V1C_CM_HD Pos position(int64_t r2, uint32_t scale, int shift)
{
    const uint64_t q = ((uint64_t)r2 * scale) >> shift;
    const uint64_t i = q >> 8;
    Pos p;
    p.idx = i >= (uint64_t)kBins ? (uint32_t)(kBins - 1) : (uint32_t)i;
    p.f = i >= (uint64_t)kBins ? 255u : (uint32_t)(q & 255u);
    return p;
}

// T: one channel's kBins + 1 entries
V1C_CM_HD uint32_t gain_q14(const uint16_t* T, Pos p)
{
    return ((uint32_t)T[p.idx] * (256u - p.f) + (uint32_t)T[p.idx + 1] * p.f + 128u) >> 8;
}

// v, G <= 65535: the product and its rounding stay below 2^32
V1C_CM_HD uint32_t scaled(uint32_t v, uint32_t G, uint32_t maxv)
{
    const uint32_t o = (v * G + (1u << 13)) >> 14;
    return o > maxv ? maxv : o;
}

// the table of channel c of a pixel with CN channels: BGR, a grey image takes green's
template <int CN>
V1C_CM_HD int table_of(int c)
{
    return CN == 1 ? 1 : c;
}

// ---- the ring statistics.  The ring of r2 < R2: (r2 * rings) / R2 -- below 2^44, never above rings - 1
V1C_CM_HD int ring_of(int64_t r2, int64_t R2, int rings)
{
    const int k = (int)((uint64_t)(r2 * rings) / (uint64_t)R2);
    return k < rings - 1 ? k : rings - 1;
}

// the merge in front of the accumulator add (k_cm_hist's): a thread keeps the ring it saw last with its partial sums, the add goes
// out when the ring changes and at the end of a round.  Near the centre row the lanes of a wave share a ring for whole segments.
struct RingRun {
    int ring = -1;
    uint32_t s[3] = {0, 0, 0};
    uint32_t n = 0;
};

// add(ring, word, value) receives what leaves the run
template <class Add>
V1C_CM_HD void ring_flush(RingRun& run, Add& add)
{
    if (run.n) {
#pragma unroll
        for (int c = 0; c < 3; c++)
            if (run.s[c])
                add(run.ring, c, run.s[c]);
        add(run.ring, 3, run.n);
    }
    run.ring = -1;
    run.s[0] = run.s[1] = run.s[2] = 0;
    run.n = 0;
}

// one pixel: v holds its CC colour channels
template <int CC, class Add>
V1C_CM_HD void ring_pixel(const int* v, int64_t r2, const RingParams& prm, RingRun& run, Add& add)
{
    bool in = r2 < prm.r2;
#pragma unroll
    for (int c = 0; c < CC; c++)
        in = in & (v[c] >= prm.lo) & (v[c] <= prm.hi);
    if (!in)
        return;
    const int ring = ring_of(r2, prm.r2, prm.rings);
    if (ring != run.ring) {
        ring_flush(run, add);
        run.ring = ring;
    }
    if (CC == 1) {
        run.s[1] += (uint32_t)v[0];
    } else {
#pragma unroll
        for (int c = 0; c < CC; c++)
            run.s[c] += (uint32_t)v[c];
    }
    run.n++;
}

// ---- the bound of the 32-bit accumulators.  An item holds at most 15 + 15 pixels (head and tail) or 16 (a segment); between two
// flushes a thread walks kFlushItems items and a wave 64 times that: 64 * 32 * 30 = 61440 pixels of at most 65535 each, below 2^32 in
// every word of the wave's copy, and 32 * 30 * 65535 below 2^26 in a thread's run.
constexpr int kFlushItems = 32;
constexpr int kItemPixelsMax = 2 * (kSegPixels - 1);
static_assert((uint64_t)64 * kFlushItems * kItemPixelsMax * 65535u < ((uint64_t)1 << 32), "a wave's copy overflows between flushes");

}  // namespace vignette
}  // namespace v1c
