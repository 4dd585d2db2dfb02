// chroma_core.hpp -- per-pixel building blocks of the lateral chromatic aberration remap (kernels_chroma.hip): one ray direction per
// output pixel, one radial table per colour channel, one channel of a BGR source sampled per coordinate.
//
// __host__ __device__ like v1c_core.hpp, whose pieces it reuses unchanged: the host tests run ray_eval3 against ray_eval.
//
// Three channel chains that differ only in radial stages in front of Denormalize share everything ray_eval computes up to m = 1 - v_z
// and the factors sx_, sy_, kx, ky; they differ in the radial table G is read from.  ray_eval3 evaluates that head once and then runs
// the tail of ray_eval -- the very operations, in the same order, under the same contraction state -- once per table, so that channel c
// gets bit for bit what ray_eval gives with a RayParams carrying table c.
#pragma once

#include "v1c_core.hpp"

namespace v1c {

// the part of RayParams a channel has of its own
struct CaTable {
    const double* radial;  // [n_int][kRadialCoefs]
    double inv_step;
    int n_int;
    int var_is_w;
};

#pragma clang fp contract(fast)  // (the state ray_eval is compiled under)

// `P`: the RayParams of the shared head (its own radial / inv_step / n_int / var_is_w are not read); `T`: the tables of B, G, R.
// True: all three channels are inside their tables and ranges -- a pixel is valid only then; the outputs of the channels evaluated so
// far are written either way.
// (`RP`, `TB`, `RotPtr`: RayParams, CaTable[3] and the 9 doubles of the rotation, or the constant-address-space views of them the
// kernels read the plan's context and the launch's units through -- like gen_vector's)
template <typename RP, typename TB, typename RotPtr>
V1C_HDF bool ray_eval3(RP& P, TB& T, bool use_rot, RotPtr rot, double sl, double cl, double hl, double slon, double clon, double hlon,
                       double (&ox)[3], double (&oy)[3])
{
    double m;
    double sx_, sy_;
    double kx, ky;
    if (P.gen_mode) {
        if (!gen_vector(P, rot, sl, cl, hl, slon, hlon, sx_, sy_, m))
            return false;
        kx = P.rx32, ky = P.ry32;
        use_rot = true;
    } else if (use_rot) {
        sx_ = fma(rot[0] * cl, slon, fma(rot[2] * cl, clon, rot[1] * sl));
        sy_ = fma(rot[3] * cl, slon, fma(rot[5] * cl, clon, rot[4] * sl));
        m = 1.0 - fma(rot[6] * cl, slon, fma(rot[8] * cl, clon, rot[7] * sl));
        kx = P.rx32, ky = P.ry32;
    } else {
        sx_ = slon, sy_ = 1.0;
        kx = P.rx32 * cl, ky = P.ry32 * sl;
        m = fma(cl, hlon, hl);
    }
    bool ok = true;
    double w = 0.0;
    bool have_w = false;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        double u = m;
        if (T[ch].var_is_w) {
            if (!have_w)
                w = fast_sqrt_half(m), have_w = true;  // (a pure function of m: evaluated once for the tables that are in w)
            u = w;
        }
        const double t = u * T[ch].inv_step;
        const int idx = table_index(t);
        if ((unsigned)idx >= (unsigned)T[ch].n_int) {
            ok = false;
            continue;
        }
        const double z = t - ((double)idx + 0.5);
        const double* c = T[ch].radial + (size_t)idx * kRadialCoefs;
        double g = c[kRadialDegree];
#pragma unroll
        for (int k = kRadialDegree - 1; k >= 0; k--)
            g = fma(g, z, c[k]);
        const double x32 = fma(g * kx, sx_, P.cx32);
        const double y32 = use_rot ? fma(g * ky, sy_, P.cy32) : fma(g, ky, P.cy32);
        if (!(fabsf((float)x32) < 1073741824.0f && fabsf((float)y32) < 1073741824.0f)) {
            ok = false;
            continue;
        }
        ox[ch] = x32 * 0.03125;
        oy[ch] = y32 * 0.03125;
    }
    return ok;
}

// ------------------------------------------------------------------------------------------
// one channel `ch` of a 3-channel uint8 source at (x, y): the byte arithmetic of sample<3, INTERP> (v1c_core.hpp) for that channel alone
// -- the same taps, weights, border decisions and rounding.  False: the byte is left as it is (BORDER_TRANSPARENT).
// ------------------------------------------------------------------------------------------
V1C_HD bool ca_nearest(const Image& s, const Geom& g, float x, float y, int ch, uint8_t& out)
{
    int sx = clamp_short(cv_round(x)), sy = clamp_short(cv_round(y));
    if (!((unsigned)sx < (unsigned)s.w && (unsigned)sy < (unsigned)s.h)) {
        if (g.border == V1C_BORDER_TRANSPARENT)
            return false;
        if (g.border == V1C_BORDER_CONSTANT) {
            out = g.cval[ch];
            return true;
        }
        sx = border_index(sx, s.w, g.border);
        sy = border_index(sy, s.h, g.border);
    }
    out = s.p[(int64_t)sy * s.pitch + (int64_t)sx * 3 + ch];
    return true;
}

V1C_HD bool ca_linear(const Image& s, const Geom& g, float x, float y, int ch, uint8_t& out)
{
    const Taps t = quantize(x, y);
    const int wx1 = t.fx, wx0 = 32 - t.fx, wy1 = t.fy, wy0 = 32 - t.fy;
    const int W = s.w, H = s.h;
    int x0, x1, y0, y1;
    if ((unsigned)t.ix < (unsigned)(W - 1) && (unsigned)t.iy < (unsigned)(H - 1)) {
        x0 = t.ix, x1 = t.ix + 1, y0 = t.iy, y1 = t.iy + 1;
    } else {
        if (g.border == V1C_BORDER_CONSTANT && (t.ix >= W || t.ix + 1 < 0 || t.iy >= H || t.iy + 1 < 0)) {
            out = g.cval[ch];
            return true;
        }
        if (g.border == V1C_BORDER_TRANSPARENT)
            return false;
        x0 = border_index(t.ix, W, g.border);
        x1 = border_index(t.ix + 1, W, g.border);
        y0 = border_index(t.iy, H, g.border);
        y1 = border_index(t.iy + 1, H, g.border);
    }
    const uint8_t* r0 = s.p + (int64_t)(y0 < 0 ? 0 : y0) * s.pitch + ch;
    const uint8_t* r1 = s.p + (int64_t)(y1 < 0 ? 0 : y1) * s.pitch + ch;
    const int cv = g.cval[ch];
    const int p00 = (x0 >= 0 && y0 >= 0) ? r0[x0 * 3] : cv;
    const int p01 = (x1 >= 0 && y0 >= 0) ? r0[x1 * 3] : cv;
    const int p10 = (x0 >= 0 && y1 >= 0) ? r1[x0 * 3] : cv;
    const int p11 = (x1 >= 0 && y1 >= 0) ? r1[x1 * 3] : cv;
    const int h0 = p00 * wx0 + p01 * wx1;
    const int h1 = p10 * wx0 + p11 * wx1;
    out = (uint8_t)((h0 * wy0 + h1 * wy1 + 512) >> 10);
    return true;
}

template <int K>
V1C_HD bool ca_table(const Image& s, const Geom& g, const short* __restrict__ itab, float x, float y, int ch, uint8_t& out)
{
    const Taps t = quantize(x, y);
    const short* __restrict__ w = itab + (size_t)(t.fy * 32 + t.fx) * (K * K);
    const int off = K / 2 - 1;
    const int sx = t.ix - off, sy = t.iy - off;
    const int W = s.w, H = s.h;
    int acc = 0;
    if ((unsigned)sx < (unsigned)(W - (K - 1) > 0 ? W - (K - 1) : 0) && (unsigned)sy < (unsigned)(H - (K - 1) > 0 ? H - (K - 1) : 0)) {
        const uint8_t* S = s.p + (int64_t)sy * s.pitch + (int64_t)sx * 3 + ch;
        for (int i = 0; i < K; i++, S += s.pitch) {
#pragma unroll
            for (int j = 0; j < K; j++)
                acc += S[j * 3] * w[i * K + j];
        }
    } else {
        int border = g.border;
        if (border == V1C_BORDER_TRANSPARENT) {
            if ((unsigned)(sx + off) >= (unsigned)W || (unsigned)(sy + off) >= (unsigned)H)
                return false;
            border = V1C_BORDER_REFLECT_101;
        }
        if (border == V1C_BORDER_CONSTANT && (sx >= W || sx + K <= 0 || sy >= H || sy + K <= 0)) {
            out = g.cval[ch];
            return true;
        }
        const int cv = g.cval[ch];
        int xs[K];
#pragma unroll
        for (int j = 0; j < K; j++)
            xs[j] = border_index(sx + j, W, border);
        for (int i = 0; i < K; i++) {
            const int yi = border_index(sy + i, H, border);
            const uint8_t* S = s.p + (int64_t)(yi < 0 ? 0 : yi) * s.pitch + ch;
#pragma unroll
            for (int j = 0; j < K; j++)
                acc += ((yi >= 0 && xs[j] >= 0) ? (int)S[xs[j] * 3] : cv) * w[i * K + j];
        }
    }
    const int v = (acc + (1 << 14)) >> 15;
    out = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
    return true;
}

template <int INTERP>
V1C_HDF bool ca_sample(const Image& s, const Geom& g, const short* itab, float x, float y, int ch, uint8_t& out)
{
    if (INTERP == V1C_INTER_NEAREST)
        return ca_nearest(s, g, x, y, ch, out);
    if (INTERP == V1C_INTER_LINEAR)
        return ca_linear(s, g, x, y, ch, out);
    if (INTERP == V1C_INTER_CUBIC)
        return ca_table<4>(s, g, itab, x, y, ch, out);
    return ca_table<8>(s, g, itab, x, y, ch, out);
}

}  // namespace v1c
