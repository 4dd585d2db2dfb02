// colormatch.hip -- host side of the colour-match entry points of the C ABI (v1c_color_match_*, v1c_apply_luts_async,
// include/vr180_remap.h): argument checks, the defaults and the launches of kernels_colormatch.hip.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/vr180_remap.h"
#include "colormatch_launch.hpp"
#include "host_util.hpp"

using namespace v1c;
using namespace v1c::colormatch;

#define CM_HIP_TRY(expr)                                                                                \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess)                                                                           \
            return set_error(V1C_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));             \
    } while (0)

namespace {

// NULL: histogram mode, the left eye as the reference, mask [10, 254], shifts within 64 levels, at least 1024 counted positions
const Params kDefaults = {kModeHistogram, V1C_CM_REFERENCE_LEFT, 10, 254, 64, 1024};

int check_image(const std::string& me, int h, int w, int cn, int64_t pitch_a, int64_t pitch_b)
{
    if (cn != 1 && cn != 3 && cn != 4)
        return set_error(V1C_E_INVALID, me + ": cn must be 1, 3 or 4");
    if (h <= 0 || w <= 0 || (int64_t)h * w >= ((int64_t)1 << 31))
        return set_error(V1C_E_INVALID, me + ": image size must be positive with h * w < 2^31");
    if (pitch_a < (int64_t)w * cn || pitch_b < (int64_t)w * cn)
        return set_error(V1C_E_INVALID, me + ": pitch below the bytes of a row");
    return V1C_OK;
}

}  // namespace

extern "C" uint64_t v1c_color_match_workspace(void) { return workspace_bytes(); }

extern "C" int v1c_color_match_luts_async(int device, void* stream, const void* left, int64_t left_pitch, const void* right,
                                          int64_t right_pitch, int h, int w, int cn, const v1c_color_match_params* params, void* workspace,
                                          uint8_t* luts_dev, int32_t* report_dev)
{
    const std::string me("v1c_color_match_luts_async");
    if (!left || !right || !workspace || !luts_dev || !report_dev)
        return set_error(V1C_E_INVALID, me + ": NULL pointer");
    int rc = check_image(me, h, w, cn, left_pitch, right_pitch);
    if (rc)
        return rc;
    if (((uintptr_t)workspace & 3) || ((uintptr_t)report_dev & 3))
        return set_error(V1C_E_INVALID, me + ": workspace and report must be 4-byte aligned");
    Params prm = kDefaults;
    if (params) {
        if ((params->mode != V1C_CM_MODE_HISTOGRAM && params->mode != V1C_CM_MODE_GAIN) ||
            (params->reference != V1C_CM_REFERENCE_LEFT && params->reference != V1C_CM_REFERENCE_RIGHT) || params->lo < 0 || params->hi > 255 ||
            params->lo > params->hi || params->max_shift < 0 || params->max_shift > 255 || params->min_pixels < 0)
            return set_error(V1C_E_INVALID, me + ": parameter out of range (mode 0 / 1, reference 0 / 1, 0 <= lo <= hi <= 255, max_shift 0..255, "
                                                 "min_pixels >= 0)");
        prm = Params{params->mode, params->reference, params->lo, params->hi, params->max_shift, params->min_pixels};
    }
    DeviceGuard dg(device);
    if (!dg.ok)
        return set_error(V1C_E_NODEVICE, "hipSetDevice failed");
    CM_HIP_TRY(launch_luts((const uint8_t*)left, left_pitch, (const uint8_t*)right, right_pitch, h, w, cn, prm, (uint32_t*)workspace, luts_dev,
                           report_dev, (hipStream_t)stream));
    return V1C_OK;
}

extern "C" int v1c_apply_luts_async(int device, void* stream, const void* src, int64_t src_pitch, void* dst, int64_t dst_pitch, int h, int w,
                                    int cn, const uint8_t* luts_dev)
{
    const std::string me("v1c_apply_luts_async");
    if (!src || !dst || !luts_dev)
        return set_error(V1C_E_INVALID, me + ": NULL pointer");
    int rc = check_image(me, h, w, cn, src_pitch, dst_pitch);
    if (rc)
        return rc;
    DeviceGuard dg(device);
    if (!dg.ok)
        return set_error(V1C_E_NODEVICE, "hipSetDevice failed");
    CM_HIP_TRY(launch_apply((const uint8_t*)src, src_pitch, (uint8_t*)dst, dst_pitch, h, w, cn, luts_dev, (hipStream_t)stream));
    return V1C_OK;
}
