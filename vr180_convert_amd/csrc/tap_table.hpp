// tap_table.hpp -- the pair mirror kernel's per-plan tap table: one entry per lane of every tile pair, 12 bytes or (large tables) 8.
// What a lane of k_ray_lin3_pair_mirror_seq derives from (plan, tile, lane) alone -- the fixed-point coordinates of its 4 pixels in the
// tile's row (sx, sy) and in the mirrored row (sx, sy2), cv2's cvRound(32 x) -- is the same for both eyes and for every call on the plan.
// plan.hip fills the table once (k_fill_tap_table, kernels_mirror.hip: the kernel's own lane_coords instantiations, so the bits are the
// same by construction) and k_ray_lin3_pair_mirror_seq_tab (12-byte entries) or k_ray_lin3_pair_mirror_seq_tab8 (compact ones) reads an
// entry where the computing kernel evaluates the map.
//
// An entry holds the coordinates relative to the box origins of the tile pair's launch record (MirrorRec, tile_device.hpp), in 1/32 px:
//   x[k]  = sx[k]  - 32 * b.x0      (the band's box has an origin of its own: the kernel adds 3 * (b.x0 - q.x0) to its tap addresses)
//   y[k]  = sy[k]  - 32 * b.y0
//   y2[k] = sy2[k] - 32 * q.y0
// each as a 12-bit base (pixel 0) and three deltas to the previous pixel: 7 bits unsigned for x (the map runs left to right; up to just
// under 4 source pixels per output pixel), 6 bits signed for y and y2.  The origins are multiples of 32, so the low five bits of a decoded
// value are the fraction of the coordinate itself.
//   w0 = x[0] | dx1 << 12 | dx2 << 19 | (dx3 & 63) << 26
//   w1 = y[0] | (dy1 & 63) << 12 | (dy2 & 63) << 18 | (dy3 & 63) << 24 | (dx3 >> 6) << 30
//   w2 = y2[0] | ... as w1, bits 30 and 31 zero
// A plan whose map does not fit these ranges somewhere (tap_entry_fits) keeps no table: every launch then evaluates the map.
//
// The compact form (TapEntry8, 8 bytes per lane): what plan.hip keeps where the 12-byte table would pass kTapCompactMinBytes -- a table
// of that size comes from HBM on every launch, and a third of the entry is redundant.  Same coordinates, same origins; two facts of the
// maps shrink them (checked on the host against the oracle's maps: C2, POLY and EQUI chains, downscales to 4x, odd radii):
//   * inside a lane the steps change slowly: with d[k] = v[k] - v[k-1], the second differences d[2] - d[1] and d[3] - d[2] are in
//     [-2, 2] for x and for y, so only the first step needs width;
//   * the mirrored row is the row reflected about the source's row centre up to the rounding of each: y[k] + y2[k] differs from its
//     nominal value by at most one.  With S the nearest integer to 64 x that centre (one number per plan) and
//     K = S - 32 * (b.y0 + q.y0) (one number per tile pair: MirrorRec::tap_k),  y2[k] = K - y[k] + e[k]  with e[k] in [-2, 1].
//   w0 = x[0] | dx1 << 12 | (ddx2 & 7) << 22 | (ddx3 & 7) << 25 | (e[0] & 3) << 28 | (e[1] & 3) << 30
//   w1 = y[0] | (dy1 & 1023) << 12 | (ddy2 & 7) << 22 | (ddy3 & 7) << 25 | (e[2] & 3) << 28 | (e[3] & 3) << 30
// 12-bit bases as above; dx1 = x[1] - x[0] 10 bits unsigned, dy1 = y[1] - y[0] 10 bits signed (the format needs 7 and 6: the seven
// bits left over widen the first steps); ddx2 = (x[2] - x[1]) - dx1 and ddx3 = (x[3] - x[2]) - (x[2] - x[1]) 3 bits signed, ddy
// likewise; e[k] 2 bits signed.  y2 has no field of its own.  tap8_fits is the rule; where it fails the plan keeps no table.
// No HIP type in here: tests/host_tap_table compiles it for the host.
#pragma once
#include <cstdint>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#define V1C_TAP_TABLE_OWN_QUALIFIERS
#endif

namespace v1c {

constexpr int kTapPX = 4;           // pixels per lane (kPX)
constexpr int kTapEntryBytes = 12;
constexpr int kTapBaseMax = 4095;   // 12 bits: boxes up to 128 px wide / high
constexpr int kTapDxMax = 127;      // 7 bits, unsigned
constexpr int kTapDyMin = -32, kTapDyMax = 31;  // 6 bits, signed

struct TapEntry {
    uint32_t w[3];
};
static_assert(sizeof(TapEntry) == kTapEntryBytes, "three dwords per lane");

struct TapCoords {
    int x[kTapPX], y[kTapPX], y2[kTapPX];
};

__host__ __device__ inline bool tap_entry_fits(const TapCoords& c)
{
    bool ok = c.x[0] >= 0 && c.x[0] <= kTapBaseMax && c.y[0] >= 0 && c.y[0] <= kTapBaseMax && c.y2[0] >= 0 && c.y2[0] <= kTapBaseMax;
    for (int k = 1; k < kTapPX; k++) {
        const int dx = c.x[k] - c.x[k - 1], dy = c.y[k] - c.y[k - 1], dy2 = c.y2[k] - c.y2[k - 1];
        ok = ok && dx >= 0 && dx <= kTapDxMax && dy >= kTapDyMin && dy <= kTapDyMax && dy2 >= kTapDyMin && dy2 <= kTapDyMax;
    }
    return ok;
}

// (values that do not fit are truncated to their fields: the caller asks tap_entry_fits)
__host__ __device__ inline TapEntry tap_entry_encode(const TapCoords& c)
{
    const uint32_t dx1 = (uint32_t)(c.x[1] - c.x[0]) & 127u, dx2 = (uint32_t)(c.x[2] - c.x[1]) & 127u, dx3 = (uint32_t)(c.x[3] - c.x[2]) & 127u;
    TapEntry e;
    e.w[0] = ((uint32_t)c.x[0] & 4095u) | dx1 << 12 | dx2 << 19 | (dx3 & 63u) << 26;
    e.w[1] = ((uint32_t)c.y[0] & 4095u) | ((uint32_t)(c.y[1] - c.y[0]) & 63u) << 12 | ((uint32_t)(c.y[2] - c.y[1]) & 63u) << 18 |
             ((uint32_t)(c.y[3] - c.y[2]) & 63u) << 24 | (dx3 >> 6) << 30;
    e.w[2] = ((uint32_t)c.y2[0] & 4095u) | ((uint32_t)(c.y2[1] - c.y2[0]) & 63u) << 12 | ((uint32_t)(c.y2[2] - c.y2[1]) & 63u) << 18 |
             ((uint32_t)(c.y2[3] - c.y2[2]) & 63u) << 24;
    return e;
}

// six bits from bit `pos` of `w`, sign-extended
__host__ __device__ inline int tap_sext6(uint32_t w, int pos)
{
    return (int)(w << (26 - pos)) >> 26;
}

__host__ __device__ inline TapCoords tap_entry_decode(const TapEntry& e)
{
    TapCoords c;
    c.x[0] = (int)(e.w[0] & 4095u);
    c.x[1] = c.x[0] + (int)((e.w[0] >> 12) & 127u);
    c.x[2] = c.x[1] + (int)((e.w[0] >> 19) & 127u);
    c.x[3] = c.x[2] + (int)((e.w[0] >> 26) | ((e.w[1] >> 30) & 1u) << 6);
    c.y[0] = (int)(e.w[1] & 4095u), c.y2[0] = (int)(e.w[2] & 4095u);
    for (int k = 1; k < kTapPX; k++) {
        c.y[k] = c.y[k - 1] + tap_sext6(e.w[1], 6 + 6 * k);
        c.y2[k] = c.y2[k - 1] + tap_sext6(e.w[2], 6 + 6 * k);
    }
    return c;
}

// ---- the compact form ----
constexpr int kTap8EntryBytes = 8;
constexpr int kTap8DxMax = 1023;                   // first step of x: 10 bits, unsigned
constexpr int kTap8DyMin = -512, kTap8DyMax = 511;  // first step of y: 10 bits, signed
constexpr int kTap8DdMin = -4, kTap8DdMax = 3;      // second differences: 3 bits, signed
constexpr int kTap8EMin = -2, kTap8EMax = 1;        // y2[k] - (K - y[k]): 2 bits, signed

struct TapEntry8 {
    uint32_t w[2];
};
static_assert(sizeof(TapEntry8) == kTap8EntryBytes, "two dwords per lane");

// `bits` bits from bit `pos` of `w`, sign-extended
__host__ __device__ inline int tap_sext(uint32_t w, int pos, int bits)
{
    return (int)(w << (32 - bits - pos)) >> (32 - bits);
}

// `K`: the tile pair's S - 32 * (b.y0 + q.y0), see above
__host__ __device__ inline bool tap8_fits(const TapCoords& c, int K)
{
    const int dx1 = c.x[1] - c.x[0], dy1 = c.y[1] - c.y[0];
    bool ok = c.x[0] >= 0 && c.x[0] <= kTapBaseMax && c.y[0] >= 0 && c.y[0] <= kTapBaseMax && dx1 >= 0 && dx1 <= kTap8DxMax &&
              dy1 >= kTap8DyMin && dy1 <= kTap8DyMax;
    for (int k = 2; k < kTapPX; k++) {
        const int ddx = (c.x[k] - c.x[k - 1]) - (c.x[k - 1] - c.x[k - 2]), ddy = (c.y[k] - c.y[k - 1]) - (c.y[k - 1] - c.y[k - 2]);
        ok = ok && ddx >= kTap8DdMin && ddx <= kTap8DdMax && ddy >= kTap8DdMin && ddy <= kTap8DdMax;
    }
    for (int k = 0; k < kTapPX; k++) {
        const int e = c.y2[k] - (K - c.y[k]);
        ok = ok && e >= kTap8EMin && e <= kTap8EMax;
    }
    return ok;
}

// (values that do not fit are truncated to their fields: the caller asks tap8_fits)
__host__ __device__ inline TapEntry8 tap8_encode(const TapCoords& c, int K)
{
    uint32_t dd[2][2], e[kTapPX];
    for (int k = 2; k < kTapPX; k++) {
        dd[0][k - 2] = (uint32_t)((c.x[k] - c.x[k - 1]) - (c.x[k - 1] - c.x[k - 2])) & 7u;
        dd[1][k - 2] = (uint32_t)((c.y[k] - c.y[k - 1]) - (c.y[k - 1] - c.y[k - 2])) & 7u;
    }
    for (int k = 0; k < kTapPX; k++)
        e[k] = (uint32_t)(c.y2[k] - (K - c.y[k])) & 3u;
    TapEntry8 o;
    o.w[0] = ((uint32_t)c.x[0] & 4095u) | ((uint32_t)(c.x[1] - c.x[0]) & 1023u) << 12 | dd[0][0] << 22 | dd[0][1] << 25 | e[0] << 28 | e[1] << 30;
    o.w[1] = ((uint32_t)c.y[0] & 4095u) | ((uint32_t)(c.y[1] - c.y[0]) & 1023u) << 12 | dd[1][0] << 22 | dd[1][1] << 25 | e[2] << 28 | e[3] << 30;
    return o;
}

__host__ __device__ inline TapCoords tap8_decode(const TapEntry8& t, int K)
{
    TapCoords c;
    const int dx1 = (int)((t.w[0] >> 12) & 1023u), dx2 = dx1 + tap_sext(t.w[0], 22, 3), dx3 = dx2 + tap_sext(t.w[0], 25, 3);
    const int dy1 = tap_sext(t.w[1], 12, 10), dy2 = dy1 + tap_sext(t.w[1], 22, 3), dy3 = dy2 + tap_sext(t.w[1], 25, 3);
    c.x[0] = (int)(t.w[0] & 4095u), c.x[1] = c.x[0] + dx1, c.x[2] = c.x[1] + dx2, c.x[3] = c.x[2] + dx3;
    c.y[0] = (int)(t.w[1] & 4095u), c.y[1] = c.y[0] + dy1, c.y[2] = c.y[1] + dy2, c.y[3] = c.y[2] + dy3;
    const int e[kTapPX] = {tap_sext(t.w[0], 28, 2), (int)t.w[0] >> 30, tap_sext(t.w[1], 28, 2), (int)t.w[1] >> 30};
    for (int k = 0; k < kTapPX; k++)
        c.y2[k] = K - c.y[k] + e[k];
    return c;
}

}  // namespace v1c

#ifdef V1C_TAP_TABLE_OWN_QUALIFIERS
#undef __host__
#undef __device__
#undef V1C_TAP_TABLE_OWN_QUALIFIERS
#endif
