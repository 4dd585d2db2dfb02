// kernels_chroma.hip -- gfx950 kernels of the lateral chromatic aberration remap: one map per colour channel of a BGR image.
//
// k_remap_ca has the launch shape of k_remap (kernels.hip): 64 x 4 lanes, kPX horizontally adjacent output pixels per lane, units on
// grid.z, a rotation per unit.  Every output byte out[.., ch] is what k_remap writes there for channel ch's own chain: the coordinates
// come from ray_eval3 (chroma_core.hpp: one ray direction, three radial tables) or from three runs of the fp64 interpreter, the byte
// from the one-channel form of the cv2.remap-exact sampler.
//
//   MODE_RAY      ray_eval3.  A pixel with ANY channel outside its table is not written; its tile is flagged and
//   MODE_FIXUP    (a second, normally empty launch) evaluates the three chains with the interpreter for exactly those pixels.
//   MODE_LITERAL  three interpreters per pixel: lowerable chains that do not fuse.
//
// Arguments: one CaArgs block by value, read -- like the plan-resident context it points to -- through constant-address-space
// references, so that every value is a scalar load next to its use.  (With CaCtx and UnitArgs as by-value parameters the compiler
// hoisted their loads to the kernel entry and kept them live: every ray-mode instantiation spilled 20 to 90 scalar registers.)
#include "chroma_launch.hpp"

namespace v1c {

#define V1C_CONST __attribute__((address_space(4)))
typedef const V1C_CONST CaCtx& ca_ctx_cref;
typedef const V1C_CONST DevUnit& ca_unit_cref;

struct CaKernelView {
    const V1C_CONST CaCtx* c;
    const V1C_CONST DevUnit* u;
};

// Every kernel of this file takes CaArgs as its FIRST parameter, by value, and reads it at byte 0 of the kernel-argument segment instead
// of through the formal parameter.  That holds because a by-value struct starts the segment at its natural alignment (8) and because
// the build's -amdgpu-kernarg-preload-count=16 (csrc/Makefile) preloads leading SCALAR arguments only: a struct in front stops it, also
// for k_get_map_ca's scalars behind the block.  tests/test_chroma_resources.py checks offset 0 in every kernel's metadata.
static_assert(offsetof(CaArgs, ctx) == 0 && offsetof(CaArgs, u) == 8 && alignof(CaArgs) == 8,
              "ca_view() reads the context pointer at byte 0 and the units at byte 8 of the kernel-argument segment");

__device__ __forceinline__ CaKernelView ca_view(int z)
{
    const V1C_CONST CaArgs* a = (const V1C_CONST CaArgs*)__builtin_amdgcn_kernarg_segment_ptr();
    return CaKernelView{(const V1C_CONST CaCtx*)a->ctx, &a->u[z]};
}

// the ray path's coordinates of the three channels at (i, j); false: some channel is outside its table
__device__ __forceinline__ bool ca_ray_coords(ca_ctx_cref c, ca_unit_cref u, int i, double sl, double cl, double hl, float (&fx)[3],
                                              float (&fy)[3])
{
    const V1C_CONST RayParams& rp = c.ray;
    const bool use_rot = u.has_rot != 0 || rp.has_rot != 0;
    double x[3], y[3];
    const bool ok = ray_eval3(rp, c.tab, use_rot, (const V1C_CONST double*)u.rot, sl, cl, hl, rp.col_s[i], rp.col_c[i], rp.col_h[i], x, y);
    if (ok) {
#pragma unroll
        for (int ch = 0; ch < 3; ch++)
            fx[ch] = (float)x[ch], fy[ch] = (float)y[ch];
    }
    return ok;
}

// ... and the interpreter's (a slow path by construction: the rotation is copied out of the argument block)
__device__ __noinline__ void ca_literal_coords(const v1c_chain* chains, const double* rot_or_null, int i, int j, float* fx, float* fy)
{
    for (int ch = 0; ch < 3; ch++) {
        double x, y;
        eval_chain_literal(chains + ch, rot_or_null, i, j, x, y);
        fx[ch] = (float)x;  // astype(np.float32), remapper.py:58
        fy[ch] = (float)y;
    }
}

template <int INTERP, int MODE>
__global__ __launch_bounds__(kBlockX* kBlockY) void k_remap_ca(CaArgs)
{
    const CaKernelView kv = ca_view(blockIdx.z);
    ca_ctx_cref c = *kv.c;
    ca_unit_cref un = *kv.u;
    const int tile = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    if (MODE == MODE_FIXUP) {
        // uniform early exit for tiles the ray pass completed; self-cleaning flag
        const uint32_t flagged = c.tile_flags[tile];
        if (!flagged)
            return;
        __syncthreads();
        if (threadIdx.x == 0 && threadIdx.y == 0)
            c.tile_flags[tile] = 0;
    }
    Geom g;
    g.src_h = c.g.src_h, g.src_w = c.g.src_w, g.dst_h = c.g.dst_h, g.dst_w = c.g.dst_w;
    g.cn = 3, g.interp = INTERP, g.border = c.g.border;
#pragma unroll
    for (int q = 0; q < 4; q++)
        g.cval[q] = c.g.cval[q];
    const int x0 = (blockIdx.x * kBlockX + threadIdx.x) * kPX;
    const int j = blockIdx.y * kBlockY + threadIdx.y;
    if (x0 >= g.dst_w || j >= g.dst_h)
        return;
    const int npx = min(kPX, g.dst_w - x0);

    double sl = 0.0, cl = 0.0, hl = 0.0;
    if (MODE != MODE_LITERAL) {
        // the row index is wave-uniform (blockDim.x == 64): the row table reads become scalar loads
        const int ju = __builtin_amdgcn_readfirstlane(j);
        sl = c.ray.row_s[ju], cl = c.ray.row_c[ju], hl = c.ray.row_h[ju];
    }
    double rot_copy[9];
    const double* rot_lit = nullptr;
    if (MODE != MODE_RAY && un.has_rot) {
#pragma unroll
        for (int q = 0; q < 9; q++)
            rot_copy[q] = un.rot[q];
        rot_lit = rot_copy;
    }

    const Image src{un.src, un.src_pitch, g.src_h, g.src_w};
    uint8_t* drow = un.dst + (int64_t)j * un.dst_pitch + (int64_t)x0 * 3;
    const short* itab = c.itab;

    // The pixel loop stays rolled (three table evaluations and three samplers per pixel).  A pixel's three bytes travel in one dword
    // picked by selects, so nothing is indexed with the loop counter.
    static_assert(kPX == 4, "the packing below is written for 4 pixels per lane");
    uint32_t p0 = 0, p1 = 0, p2 = 0, p3 = 0;
    unsigned written = 0;  // one bit per byte of the lane's 12
    bool all_valid = true;
#pragma nounroll
    for (int k = 0; k < npx; k++) {
        float fx[3], fy[3];
        bool go = true;
        if (MODE != MODE_LITERAL) {
            const bool ok = ca_ray_coords(c, un, x0 + k, sl, cl, hl, fx, fy);
            go = MODE == MODE_RAY ? ok : !ok;  // fix-up: exactly the pixels the ray pass left
            all_valid &= ok;
        }
        if (MODE != MODE_RAY && go)
            ca_literal_coords(c.chains, rot_lit, x0 + k, j, fx, fy);
        uint32_t v3 = 0;
        unsigned w3 = 0;
        if (go && INTERP == V1C_INTER_LANCZOS4) {
            // (one copy of the 8 x 8 sampler: three of them cost the ray-mode instantiation 19 spilled scalar registers)
#pragma nounroll
            for (int ch = 0; ch < 3; ch++) {
                const float x = ch == 0 ? fx[0] : (ch == 1 ? fx[1] : fx[2]), y = ch == 0 ? fy[0] : (ch == 1 ? fy[1] : fy[2]);
                uint8_t v = 0;
                if (ca_sample<INTERP>(src, g, itab, x, y, ch, v)) {
                    w3 |= 1u << ch;
                    v3 |= (uint32_t)v << (8 * ch);
                }
            }
        } else if (go) {
#pragma unroll
            for (int ch = 0; ch < 3; ch++) {
                uint8_t v = 0;
                if (ca_sample<INTERP>(src, g, itab, fx[ch], fy[ch], ch, v)) {
                    w3 |= 1u << ch;
                    v3 |= (uint32_t)v << (8 * ch);
                }
            }
        }
        p0 = k == 0 ? v3 : p0, p1 = k == 1 ? v3 : p1, p2 = k == 2 ? v3 : p2, p3 = k == 3 ? v3 : p3;
        written |= w3 << (3 * k);
    }
    if (MODE == MODE_RAY && !all_valid)
        c.tile_flags[tile] = 1;
    const uint32_t words[kPX * 3 / 4] = {p0 | (p1 << 24), (p1 >> 8) | (p2 << 16), (p2 >> 16) | (p3 << 8)};

    if (written == (1u << (kPX * 3)) - 1 && (((uintptr_t)drow) & 3) == 0) {
#pragma unroll
        for (int q = 0; q < kPX * 3 / 4; q++)
            ((uint32_t*)drow)[q] = words[q];
    } else {
        // ragged right edge, BORDER_TRANSPARENT holes (channel by channel), fix-up pixels, unaligned destination
#pragma unroll
        for (int b = 0; b < kPX * 3; b++) {
            if (written & (1u << b))
                drow[b] = (uint8_t)(words[b / 4] >> (8 * (b % 4)));
        }
    }
}

// the coordinate map of one channel (v1c_ca_plan_get_map): what k_remap_ca samples that channel at -- the ray path's coordinates where
// the pixel is valid (all three channels), the interpreter's elsewhere
template <int MODE>
__global__ __launch_bounds__(kBlockX* kBlockY) void k_get_map_ca(CaArgs, int channel, float* xmap, float* ymap, int64_t pitch)
{
    const CaKernelView kv = ca_view(0);
    ca_ctx_cref c = *kv.c;
    ca_unit_cref un = *kv.u;
    const int dst_w = c.g.dst_w;
    const int x0 = (blockIdx.x * kBlockX + threadIdx.x) * kPX;
    const int j = blockIdx.y * kBlockY + threadIdx.y;
    if (x0 >= dst_w || j >= c.g.dst_h)
        return;
    double sl = 0.0, cl = 0.0, hl = 0.0;
    if (MODE == MODE_RAY)
        sl = c.ray.row_s[j], cl = c.ray.row_c[j], hl = c.ray.row_h[j];
    double rot_copy[9];
    const double* rot_lit = nullptr;
    if (un.has_rot) {
        for (int q = 0; q < 9; q++)
            rot_copy[q] = un.rot[q];
        rot_lit = rot_copy;
    }
    float* xr = (float*)((char*)xmap + (int64_t)j * pitch);
    float* yr = (float*)((char*)ymap + (int64_t)j * pitch);
    for (int k = 0; k < kPX && x0 + k < dst_w; k++) {
        float fx[3], fy[3];
        bool have = false;
        if (MODE == MODE_RAY)
            have = ca_ray_coords(c, un, x0 + k, sl, cl, hl, fx, fy);
        if (!have)
            ca_literal_coords(c.chains, rot_lit, x0 + k, j, fx, fy);
        xr[x0 + k] = channel == 0 ? fx[0] : (channel == 1 ? fx[1] : fx[2]);
        yr[x0 + k] = channel == 0 ? fy[0] : (channel == 1 ? fy[1] : fy[2]);
    }
}

// ------------------------------------------------------------------------------------------
// host-callable launchers (chroma.hip)
// ------------------------------------------------------------------------------------------
static dim3 ca_grid_for(const Geom& g, int n_units)
{
    return dim3((g.dst_w + kBlockX * kPX - 1) / (kBlockX * kPX), (g.dst_h + kBlockY - 1) / kBlockY, n_units);
}

template <int MODE>
static hipError_t launch_ca_interp(const CaCtx& c, const CaArgs& a, int n_units, hipStream_t stream)
{
    const dim3 block(kBlockX, kBlockY, 1);
    const dim3 grid = ca_grid_for(c.g, n_units);
    switch (c.g.interp) {
    case V1C_INTER_NEAREST:
        hipLaunchKernelGGL((k_remap_ca<V1C_INTER_NEAREST, MODE>), grid, block, 0, stream, a);
        break;
    case V1C_INTER_LINEAR:
        hipLaunchKernelGGL((k_remap_ca<V1C_INTER_LINEAR, MODE>), grid, block, 0, stream, a);
        break;
    case V1C_INTER_CUBIC:
        hipLaunchKernelGGL((k_remap_ca<V1C_INTER_CUBIC, MODE>), grid, block, 0, stream, a);
        break;
    case V1C_INTER_LANCZOS4:
        hipLaunchKernelGGL((k_remap_ca<V1C_INTER_LANCZOS4, MODE>), grid, block, 0, stream, a);
        break;
    default:
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_remap_ca(int mode, const CaCtx& c, const CaArgs& a, int n_units, hipStream_t stream)
{
    if (n_units < 1 || n_units > kMaxUnitsPerLaunch || !a.ctx)
        return hipErrorInvalidValue;
    switch (mode) {
    case MODE_LITERAL: return launch_ca_interp<MODE_LITERAL>(c, a, n_units, stream);
    case MODE_RAY: return launch_ca_interp<MODE_RAY>(c, a, n_units, stream);
    case MODE_FIXUP: return launch_ca_interp<MODE_FIXUP>(c, a, n_units, stream);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_get_map_ca(int mode, const CaCtx& c, const CaArgs& a, int channel, float* xmap, float* ymap, int64_t pitch,
                             hipStream_t stream)
{
    if (!a.ctx)
        return hipErrorInvalidValue;
    const dim3 block(kBlockX, kBlockY, 1);
    const dim3 grid = ca_grid_for(c.g, 1);
    if (mode == MODE_RAY)
        hipLaunchKernelGGL((k_get_map_ca<MODE_RAY>), grid, block, 0, stream, a, channel, xmap, ymap, pitch);
    else
        hipLaunchKernelGGL((k_get_map_ca<MODE_LITERAL>), grid, block, 0, stream, a, channel, xmap, ymap, pitch);
    return hipGetLastError();
}

}  // namespace v1c
