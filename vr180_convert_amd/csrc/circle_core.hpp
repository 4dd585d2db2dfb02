// circle_core.hpp -- the arithmetic of the image-circle fit (v1c_fit_circle*; tests/circle_ref.py restates
// it), shared by the kernels (kernels_circle.hip) and by the host emulation (tests/host_circle/circle_emul.hip): the lit test, the
// run search within one 64-pixel step, the exact selection test, the integer residual and the float64 solve of the moment sums.
// Everything up to the solve is integer arithmetic; the solve is ONE written-out sequence of float64 operations without contraction.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define V1C_CIRCLE_HD __host__ __device__ inline
#else
#define V1C_CIRCLE_HD inline
#endif

namespace v1c {
namespace circle {

constexpr int kMaxRun = 64;     // a run crosses at most one boundary between two 64-pixel steps
constexpr int kMaxRounds = 8;
constexpr int kSums = 9;        // N, Sx, Sy, Sxx, Sxy, Syy, Sxz, Syz, Sz with z = x^2 + y^2
constexpr uint32_t kNoPoint = 0xFFFFFFFFu;

// what v1c_circle_params resolves to (include/vr180_remap.h)
struct Params {
    int32_t threshold, run, rounds, min_points;
    int32_t tol16[kMaxRounds];  // selection tolerance of round k in 1/16 px
};

// a rim point in its slot: x in the low half, y in the high half (both < 32768)
V1C_CIRCLE_HD uint32_t pack_point(int x, int y) { return (uint32_t)x | ((uint32_t)y << 16); }

// bit i of the result: the `run` pixels that END at pixel i of this step are all lit.  `m`: the step's lit mask (bit i = pixel i in scan
// order), `pm`: the mask of the step before it (0 in front of the first).  1 <= run <= 64.
V1C_CIRCLE_HD uint64_t run_ends(uint64_t m, uint64_t pm, int run)
{
    uint64_t t = m;
    for (int k = 1; k < run; k++)
        t &= (m << k) | (pm >> (64 - k));
    return t;
}

V1C_CIRCLE_HD int ctz64(uint64_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __ffsll((unsigned long long)v) - 1;
#else
    return __builtin_ctzll(v);
#endif
}

// ---- columns: every strip of 64 columns is cut into bands of kBandRows rows that are scanned independently; a column's record of a
// band says all that the search across bands needs, and the join walks the records, not the pixels
constexpr int kBandRows = 64;  // >= kMaxRun: a run crosses any number of all-lit bands, but completes within two partly lit ones

struct BandScan {
    int cnt = 0;        // lit pixels in a row up to here
    int lead = -1;      // lit pixels at the band's top (-1: all lit so far)
    int first_in = -1;  // first row of the first run that lies within the band
    int last_in = -1;   // last row of the last one
};

V1C_CIRCLE_HD void band_step(BandScan& b, bool lit, int o, int run)
{
    if (lit) {
        b.cnt++;
    } else {
        if (b.lead < 0)
            b.lead = o;
        b.cnt = 0;
    }
    if (b.cnt >= run) {
        if (b.first_in < 0)
            b.first_in = o - run + 1;
        b.last_in = o;
    }
}

// lead | trail << 7 | (first_in + 1) << 14 | (last_in + 1) << 21 of a band of `rows` rows
V1C_CIRCLE_HD uint32_t band_pack(const BandScan& b, int rows)
{
    const int lead = b.lead < 0 ? rows : b.lead;
    return (uint32_t)lead | ((uint32_t)b.cnt << 7) | ((uint32_t)(b.first_in + 1) << 14) | ((uint32_t)(b.last_in + 1) << 21);
}

struct ColJoin {
    int carry = 0;   // lit pixels in a row that touch the boundary to the next band
    int mark = 0;    // where that run began (seen from the side the walk comes from)
    int found = -1;  // the first pixel of the first run, once there is one
};

// one band of the walk down (`down`: from the top) or up.  base: the band's first row; rows: its rows; rec: band_pack's.
V1C_CIRCLE_HD void join_step(ColJoin& j, uint32_t rec, int base, int rows, int run, bool down)
{
    const int lead = (int)(rec & 127u), trail = (int)((rec >> 7) & 127u);
    const int first_in = (int)((rec >> 14) & 127u) - 1, last_in = (int)((rec >> 21) & 127u) - 1;
    const int near = down ? lead : trail, far = down ? trail : lead;  // lit pixels at the side the walk enters / leaves by
    if (j.found < 0) {
        if (j.carry > 0 && j.carry + near >= run)
            j.found = j.mark;
        else if (first_in >= 0)
            j.found = base + (down ? first_in : last_in);
    }
    if (lead == rows) {  // all lit: the run goes on
        if (j.carry == 0)
            j.mark = down ? base : base + rows - 1;
        j.carry += rows;
    } else {
        j.carry = far;
        j.mark = down ? base + rows - far : base + far - 1;
    }
}

// floor(sqrt(v)) for 0 <= v < 2^52, exact: the float64 root is only a first guess
V1C_CIRCLE_HD int64_t isqrt64(int64_t v)
{
    int64_t s = (int64_t)__builtin_sqrt((double)v);
    while (s * s > v)
        s--;
    while ((s + 1) * (s + 1) <= v)
        s++;
    return s;
}

// squared distance of pixel (x, y) (relative to (W / 2, H / 2)) from the quantised centre, in (1/16 px)^2
V1C_CIRCLE_HD int64_t dist2_16(int x, int y, int64_t cx16, int64_t cy16)
{
    const int64_t dx = 16 * (int64_t)x - cx16, dy = 16 * (int64_t)y - cy16;
    return dx * dx + dy * dy;
}

// the selection test: r16 - t16 <= distance <= r16 + t16, on the squares
V1C_CIRCLE_HD bool selected(int64_t d2, int64_t r16, int64_t t16)
{
    const int64_t hi = r16 + t16, lo = r16 - t16;
    return d2 <= hi * hi && (lo <= 0 || d2 >= lo * lo);
}

struct Fit {
    double cx, cy, r;  // centre relative to (W / 2, H / 2)
    int status;        // 0, or 2 (singular) / 3 (radius or centre out of range)
};

#pragma clang fp contract(off)

// round to 1/16 px, half up
V1C_CIRCLE_HD int64_t q16(double v) { return (int64_t)__builtin_floor(v * 16.0 + 0.5); }

// Kasa's algebraic fit from the moment sums: minimise sum (z + D x + E y + F)^2.  With u = x - mean(x), v = y - mean(y):
//   [Suu Suv] [D]     [Suz]
//   [Suv Svv] [E] = - [Svz],   centre = -(D, E) / 2,   r^2 = cx^2 + cy^2 + Sz / N - 2 cx mean(x) - 2 cy mean(y)
V1C_CIRCLE_HD Fit solve(const int64_t* s, int h, int w)
{
    Fit f{0.0, 0.0, 0.0, 2};
    const double n = (double)s[0];
    if (!(n > 0.0))
        return f;
    const double sx = (double)s[1], sy = (double)s[2], sxx = (double)s[3], sxy = (double)s[4], syy = (double)s[5];
    const double sxz = (double)s[6], syz = (double)s[7], sz = (double)s[8];
    const double mx = sx / n, my = sy / n;
    const double suu = sxx - sx * mx, suv = sxy - sx * my, svv = syy - sy * my;
    const double suz = sxz - sz * mx, svz = syz - sz * my;
    const double det = suu * svv - suv * suv;
    if (!(det > 1e-12 * (suu * svv)))
        return f;
    const double cx = (suz * svv - svz * suv) / (2.0 * det);
    const double cy = (svz * suu - suz * suv) / (2.0 * det);
    const double r2 = ((cx * cx + cy * cy) + sz / n) - (2.0 * cx * mx + 2.0 * cy * my);
    const double lim = (double)(h > w ? h : w);
    f.status = 3;
    if (!(r2 > 0.0))
        return f;
    const double r = __builtin_sqrt(r2);
    if (!(r <= 4.0 * lim) || !(__builtin_fabs(cx) <= 8.0 * lim) || !(__builtin_fabs(cy) <= 8.0 * lim))
        return f;
    f.cx = cx;
    f.cy = cy;
    f.r = r;
    f.status = 0;
    return f;
}

// rms of the quantised residuals: sqrt(se2 / n) / 16 with se2 = sum (isqrt(d2) - r16)^2
V1C_CIRCLE_HD double rms16(int64_t se2, int64_t n) { return n > 0 ? __builtin_sqrt((double)se2 / (double)n) / 16.0 : 0.0; }

}  // namespace circle
}  // namespace v1c
