// wide_emul.hip -- TEST HARNESS: runs the product's 16-bit / float32 sampler (v1c_core.hpp: sample_wide) on the CPU.
//
// Built by tests/test_wide_host.py itself (hipcc --cuda-host-only -O2 -shared -fPIC, into a temporary directory) and compared there
// with the NumPy restatement of the contract (tests/wide_ref.py).  Not part of the product: nothing in vr180_convert_amd/ loads it.
#include <cstring>

#include "../../vr180_convert_amd/csrc/v1c_core.hpp"

using namespace v1c;

template <typename T, int CN>
static void remap_t(const Image& s, const Geom& g, const float* cval, const float* ftab, const float* xm, const float* ym, uint8_t* dst,
                    int64_t dst_pitch)
{
    for (int j = 0; j < g.dst_h; j++)
        for (int i = 0; i < g.dst_w; i++) {
            T px[4] = {0, 0, 0, 0};
            const float x = xm[(size_t)j * g.dst_w + i], y = ym[(size_t)j * g.dst_w + i];
            bool wr;
            switch (g.interp) {
            case V1C_INTER_NEAREST: wr = sample_wide<T, CN, V1C_INTER_NEAREST>(s, g, cval, ftab, x, y, px); break;
            case V1C_INTER_LINEAR: wr = sample_wide<T, CN, V1C_INTER_LINEAR>(s, g, cval, ftab, x, y, px); break;
            case V1C_INTER_CUBIC: wr = sample_wide<T, CN, V1C_INTER_CUBIC>(s, g, cval, ftab, x, y, px); break;
            default: wr = sample_wide<T, CN, V1C_INTER_LANCZOS4>(s, g, cval, ftab, x, y, px); break;
            }
            if (wr)
                std::memcpy(dst + (int64_t)j * dst_pitch + (int64_t)i * CN * sizeof(T), px, CN * sizeof(T));
        }
}

template <typename T>
static int remap_cn(const Image& s, const Geom& g, const float* cval, const float* ftab, const float* xm, const float* ym, uint8_t* dst,
                    int64_t dst_pitch)
{
    switch (g.cn) {
    case 1: remap_t<T, 1>(s, g, cval, ftab, xm, ym, dst, dst_pitch); return 0;
    case 3: remap_t<T, 3>(s, g, cval, ftab, xm, ym, dst, dst_pitch); return 0;
    case 4: remap_t<T, 4>(s, g, cval, ftab, xm, ym, dst, dst_pitch); return 0;
    default: return -1;
    }
}

// `depth`: 2 (uint16) or 5 (float32); pitches in bytes; maps (dst_h, dst_w) contiguous; `cval` the saturated border colour;
// `ftab` v1c_build_ftab's table of `interp` (CUBIC / LANCZOS4; may be null otherwise).  AREA is LINEAR, as in the plan.
extern "C" int wide_remap_host(const void* src, int src_h, int src_w, int64_t src_pitch, int cn, int depth, void* dst, int dst_h, int dst_w,
                               int64_t dst_pitch, const float* xmap, const float* ymap, int interp, int border, const float* cval,
                               const float* ftab)
{
    const Image s{(const uint8_t*)src, src_pitch, src_h, src_w};
    Geom g{};
    g.src_h = src_h, g.src_w = src_w, g.dst_h = dst_h, g.dst_w = dst_w, g.cn = cn, g.border = border;
    g.interp = interp == V1C_INTER_AREA ? V1C_INTER_LINEAR : interp;
    if (depth == V1C_DEPTH_16U)
        return remap_cn<uint16_t>(s, g, cval, ftab, xmap, ymap, (uint8_t*)dst, dst_pitch);
    if (depth == V1C_DEPTH_32F)
        return remap_cn<float>(s, g, cval, ftab, xmap, ymap, (uint8_t*)dst, dst_pitch);
    return -1;
}

// the product's saturation of a border Scalar (v1c_core.hpp: border_component) for `depth`: out[4] floats
extern "C" void wide_border_host(int depth, const double* bv, float* out)
{
    for (int k = 0; k < 4; k++)
        out[k] = border_component(depth, bv[k]);
}
