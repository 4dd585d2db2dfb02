// kernels_wide.hip -- cv2.remap of 16-bit unsigned (CV_16U) and float32 (CV_32F) images: k_remap_wide.
//
// The same launch shape and coordinate producers as the generic uint8 kernel k_remap (kernels.hip; coords.hpp): 64 x 4 lanes per
// workgroup, kPX output pixels per lane, one launch for up to kMaxUnitsPerLaunch units on grid.z, the MODE_RAY -> MODE_FIXUP tile-flag
// protocol unchanged.  Only the sampler differs: OpenCV's float-weight arithmetic (v1c_core.hpp: sample_wide) instead of the 5-bit
// fixed-point one.  A code object of its own: a process that only remaps uint8 images never loads these kernels.
#include "coords.hpp"

namespace v1c {

template <typename T, int CN, int INTERP, int MODE>
__global__ __launch_bounds__(kBlockX* kBlockY) void k_remap_wide(KernelCtx c, UnitArgs ua, WideArgs wa)
{
    const UnitView u = load_unit(ua, c.ray, blockIdx.z);
    const Geom& g = c.g;
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
    const int x0 = (blockIdx.x * kBlockX + threadIdx.x) * kPX;
    const int j = blockIdx.y * kBlockY + threadIdx.y;
    if (x0 >= g.dst_w || j >= g.dst_h)
        return;

    float fx[kPX], fy[kPX];
    const unsigned npx_mask = (1u << min(kPX, g.dst_w - x0)) - 1;
    const unsigned valid = Coords<MODE>::eval(c, u, x0, j, fx, fy) & npx_mask;
    if (MODE == MODE_RAY && valid != npx_mask)
        c.tile_flags[tile] = 1;

    const Image src{u.src, u.src_pitch, g.src_h, g.src_w};
    T px[kPX * CN];
    unsigned written = 0;
#pragma unroll
    for (int k = 0; k < kPX; k++) {
#pragma unroll
        for (int ch = 0; ch < CN; ch++)
            px[k * CN + ch] = 0;
        if ((valid & (1u << k)) && sample_wide<T, CN, INTERP>(src, g, wa.cval, wa.ftab, fx[k], fy[k], &px[k * CN]))
            written |= 1u << k;
    }
    T* drow = (T*)(u.dst + (int64_t)j * u.dst_pitch) + (int64_t)x0 * CN;
    constexpr int kWords = kPX * CN * (int)sizeof(T) / 4;  // (2 .. 16 dwords: every CN, both pixel types)
    if (written == (1u << kPX) - 1 && (((uintptr_t)drow) & 3) == 0) {
        uint32_t words[kWords];
        __builtin_memcpy(words, px, sizeof(words));
#pragma unroll
        for (int q = 0; q < kWords; q++)
            ((uint32_t*)drow)[q] = words[q];
    } else {
        // ragged right edge, BORDER_TRANSPARENT holes, fix-up pixels, a destination that is only 2-byte aligned
#pragma unroll
        for (int k = 0; k < kPX; k++) {
            if (written & (1u << k)) {
#pragma unroll
                for (int ch = 0; ch < CN; ch++)
                    drow[k * CN + ch] = px[k * CN + ch];
            }
        }
    }
}

template <typename T, int CN, int MODE>
static hipError_t launch_wide_interp(const KernelCtx& c, const UnitArgs& ua, const WideArgs& wa, int n_units, hipStream_t stream)
{
    const dim3 block(kBlockX, kBlockY, 1);
    const dim3 grid((c.g.dst_w + kBlockX * kPX - 1) / (kBlockX * kPX), (c.g.dst_h + kBlockY - 1) / kBlockY, n_units);  // = k_remap's
    switch (c.g.interp) {
    case V1C_INTER_NEAREST:
        hipLaunchKernelGGL((k_remap_wide<T, CN, V1C_INTER_NEAREST, MODE>), grid, block, 0, stream, c, ua, wa);
        break;
    case V1C_INTER_LINEAR:
        hipLaunchKernelGGL((k_remap_wide<T, CN, V1C_INTER_LINEAR, MODE>), grid, block, 0, stream, c, ua, wa);
        break;
    case V1C_INTER_CUBIC:
        hipLaunchKernelGGL((k_remap_wide<T, CN, V1C_INTER_CUBIC, MODE>), grid, block, 0, stream, c, ua, wa);
        break;
    case V1C_INTER_LANCZOS4:
        hipLaunchKernelGGL((k_remap_wide<T, CN, V1C_INTER_LANCZOS4, MODE>), grid, block, 0, stream, c, ua, wa);
        break;
    default:
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

template <typename T, int MODE>
static hipError_t launch_wide_cn(const KernelCtx& c, const UnitArgs& ua, const WideArgs& wa, int n_units, hipStream_t stream)
{
    switch (c.g.cn) {
    case 1: return launch_wide_interp<T, 1, MODE>(c, ua, wa, n_units, stream);
    case 3: return launch_wide_interp<T, 3, MODE>(c, ua, wa, n_units, stream);
    case 4: return launch_wide_interp<T, 4, MODE>(c, ua, wa, n_units, stream);
    default: return hipErrorInvalidValue;
    }
}

template <typename T>
static hipError_t launch_wide_mode(int mode, const KernelCtx& c, const UnitArgs& ua, const WideArgs& wa, int n_units, hipStream_t stream)
{
    switch (mode) {
    case MODE_LITERAL: return launch_wide_cn<T, MODE_LITERAL>(c, ua, wa, n_units, stream);
    case MODE_RAY: return launch_wide_cn<T, MODE_RAY>(c, ua, wa, n_units, stream);
    case MODE_FIXUP: return launch_wide_cn<T, MODE_FIXUP>(c, ua, wa, n_units, stream);
    case MODE_LUT: return launch_wide_cn<T, MODE_LUT>(c, ua, wa, n_units, stream);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_remap_wide(int mode, int depth, const KernelCtx& c, const UnitArgs& ua, const WideArgs& wa, int n_units, hipStream_t stream)
{
    switch (depth) {
    case V1C_DEPTH_16U: return launch_wide_mode<uint16_t>(mode, c, ua, wa, n_units, stream);
    case V1C_DEPTH_32F: return launch_wide_mode<float>(mode, c, ua, wa, n_units, stream);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace v1c
