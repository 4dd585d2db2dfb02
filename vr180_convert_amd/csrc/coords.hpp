// coords.hpp -- the per-pixel coordinate producers of the generic kernels: k_remap (kernels.hip, uint8) and k_remap_wide
// (kernels_wide.hip, 16-bit / float32 pixels) feed their samplers from the same code.
//
//   MODE_LITERAL  fp64 interpreter of the lowered chain (any lowerable chain)
//   MODE_RAY      separable tables + radial table.  Pixels outside the table's validated domain
//                 are NOT written; their tile is flagged and
//   MODE_FIXUP    (a second, normally empty launch) re-evaluates exactly those pixels with the
//                 interpreter.  Keeping the interpreter out of MODE_RAY keeps its register
//                 footprint small.
//   MODE_LUT      caller-supplied float32 maps (v1c_remap_lut / v1c_remap_lut_ex)
#pragma once

#include "kernels.hpp"

namespace v1c {

// Per-unit data pulled out of the kernel-argument block into registers.  (Taking the address of
// anything inside UnitArgs would make the compiler spill the whole 2 KB argument block to scratch.)
struct UnitView {
    const uint8_t* src;
    uint8_t* dst;
    int64_t src_pitch, dst_pitch;
    double rot[9];
    bool has_rot;       // the unit overrides the chain's first rotation
    bool use_rot;       // a rotation applies in ray mode (unit's or the chain's composed one)
};

__device__ __forceinline__ UnitView load_unit(const UnitArgs& ua, const RayParams& rp, int z)
{
    UnitView v;
    v.src = ua.u[z].src;
    v.dst = ua.u[z].dst;
    v.src_pitch = ua.u[z].src_pitch;
    v.dst_pitch = ua.u[z].dst_pitch;
    v.has_rot = ua.u[z].has_rot != 0;
    v.use_rot = v.has_rot || rp.has_rot;
#pragma unroll
    for (int q = 0; q < 9; q++)
        v.rot[q] = v.has_rot ? ua.u[z].rot[q] : rp.rot[q];
    return v;
}

template <int MODE>
struct Coords;

template <>
struct Coords<MODE_LITERAL> {
    __device__ static unsigned eval(const KernelCtx& c, const UnitView& u, int x0, int j, float* fx, float* fy)
    {
        const double* rot = u.has_rot ? u.rot : nullptr;
        for (int k = 0; k < kPX; k++) {
            double x, y;
            eval_chain_literal(c.chain, rot, x0 + k, j, x, y);
            fx[k] = (float)x;  // astype(np.float32), remapper.py:58
            fy[k] = (float)y;
        }
        return (1u << kPX) - 1;
    }
};

template <>
struct Coords<MODE_RAY> {
    __device__ static unsigned eval(const KernelCtx& c, const UnitView& u, int x0, int j, float* fx, float* fy)
    {
        const RayParams& rp = c.ray;
        // the row index is wave-uniform (blockDim.x == 64): tell the compiler, so the row table
        // reads become scalar loads
        const int ju = __builtin_amdgcn_readfirstlane(j);
        const double sl = rp.row_s[ju], cl = rp.row_c[ju], hl = rp.row_h[ju];
        unsigned ok = 0;
#pragma unroll
        for (int k = 0; k < kPX; k++) {
            const int i = min(x0 + k, c.g.dst_w - 1);
            double x, y;
            if (ray_eval(rp, u.use_rot, u.rot, sl, cl, hl, rp.col_s[i], rp.col_c[i], rp.col_h[i], x, y)) {
                fx[k] = (float)x;
                fy[k] = (float)y;
                ok |= 1u << k;
            }
        }
        return ok;
    }
};

template <>
struct Coords<MODE_FIXUP> {
    __device__ static unsigned eval(const KernelCtx& c, const UnitView& u, int x0, int j, float* fx, float* fy)
    {
        float rx[kPX], ry[kPX];
        const unsigned ok = Coords<MODE_RAY>::eval(c, u, x0, j, rx, ry);
        const double* rot = u.has_rot ? u.rot : nullptr;
        unsigned todo = ~ok & ((1u << kPX) - 1);
        for (int k = 0; k < kPX; k++) {
            if (todo & (1u << k)) {
                double x, y;
                eval_chain_literal(c.chain, rot, min(x0 + k, c.g.dst_w - 1), j, x, y);
                fx[k] = (float)x;
                fy[k] = (float)y;
            }
        }
        return todo;
    }
};

template <>
struct Coords<MODE_LUT> {
    __device__ static unsigned eval(const KernelCtx& c, const UnitView&, int x0, int j, float* fx, float* fy)
    {
        const float* xr = (const float*)((const char*)c.xmap + (int64_t)j * c.map_pitch);
        const float* yr = (const float*)((const char*)c.ymap + (int64_t)j * c.map_pitch);
#pragma unroll
        for (int k = 0; k < kPX; k++) {
            const int i = min(x0 + k, c.g.dst_w - 1);
            fx[k] = xr[i];
            fy[k] = yr[i];
        }
        return (1u << kPX) - 1;
    }
};

}  // namespace v1c
