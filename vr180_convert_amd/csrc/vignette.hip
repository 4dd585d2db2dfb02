// vignette.hip -- host side of the vignetting entry points of the C ABI (v1c_vignette_apply_async, v1c_vignette_rings_async,
// include/vr180_remap.h): argument checks and the launches of kernels_vignette.hip.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/vr180_remap.h"
#include "host_util.hpp"
#include "vignette_launch.hpp"

using namespace v1c;
using namespace v1c::vignette;

#define VIG_HIP_TRY(expr)                                                                               \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess)                                                                           \
            return set_error(V1C_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));             \
    } while (0)

namespace {

// what both entries ask of an image and of the circle's centre: the squared distance of every pixel stays below 2^34
int check_image(const std::string& me, int h, int w, int cn, int es, int64_t pitch, const void* base, int cx, int cy)
{
    if (cn != 1 && cn != 3 && cn != 4)
        return set_error(V1C_E_INVALID, me + ": cn must be 1, 3 or 4");
    if (es != 1 && es != 2)
        return set_error(V1C_E_INVALID, me + ": elem_bytes must be 1 (uint8) or 2 (uint16)");
    if (h <= 0 || w <= 0 || h > 32767 || w > 32767)
        return set_error(V1C_E_INVALID, me + ": image size must be within 1..32767 each way");
    if (pitch < (int64_t)w * cn * es)
        return set_error(V1C_E_INVALID, me + ": pitch below the bytes of a row");
    if (((uintptr_t)base | (uint64_t)pitch) & (uint64_t)(es - 1))
        return set_error(V1C_E_INVALID, me + ": pointers and pitches must be aligned to the element");
    if (cx < -w || cx >= 2 * w || cy < -h || cy >= 2 * h)
        return set_error(V1C_E_INVALID, me + ": the centre must lie within one frame size of the frame");
    return V1C_OK;
}

}  // namespace

extern "C" int v1c_vignette_apply_async(int device, void* stream, const void* src, int64_t src_pitch, void* dst, int64_t dst_pitch, int h,
                                        int w, int cn, int elem_bytes, const v1c_vignette_geom* geom, const uint16_t* tables_dev)
{
    const std::string me("v1c_vignette_apply_async");
    if (!src || !dst || !geom || !tables_dev)
        return set_error(V1C_E_INVALID, me + ": NULL pointer");
    int rc = check_image(me, h, w, cn, elem_bytes, src_pitch, src, geom->cx, geom->cy);
    if (rc)
        return rc;
    rc = check_image(me, h, w, cn, elem_bytes, dst_pitch, dst, geom->cx, geom->cy);
    if (rc)
        return rc;
    if ((uintptr_t)tables_dev & 1)
        return set_error(V1C_E_INVALID, me + ": tables must be 2-byte aligned");
    if (geom->scale == 0 || geom->scale >= (1u << kScaleBits) || geom->shift < 0 || geom->shift > 62)
        return set_error(V1C_E_INVALID, me + ": geometry out of range (0 < scale < 2^30, 0 <= shift <= 62)");
    static_assert(2 * ((int64_t)65534 * 65534) < ((int64_t)1 << kR2Bits), "r2 of the farthest pixel the checks let through");
    DeviceGuard dg(device);
    if (!dg.ok)
        return set_error(V1C_E_NODEVICE, "hipSetDevice failed");
    const Geom g{geom->cx, geom->cy, geom->scale, geom->shift};
    VIG_HIP_TRY(launch_apply((const uint8_t*)src, src_pitch, (uint8_t*)dst, dst_pitch, h, w, cn, elem_bytes, g, tables_dev, (hipStream_t)stream));
    return V1C_OK;
}

extern "C" int v1c_vignette_rings_async(int device, void* stream, const void* src, int64_t src_pitch, int h, int w, int cn, int elem_bytes,
                                        const v1c_vignette_ring_params* params, int64_t* rings_dev)
{
    const std::string me("v1c_vignette_rings_async");
    if (!src || !params || !rings_dev)
        return set_error(V1C_E_INVALID, me + ": NULL pointer");
    int rc = check_image(me, h, w, cn, elem_bytes, src_pitch, src, params->cx, params->cy);
    if (rc)
        return rc;
    if ((uintptr_t)rings_dev & 7)
        return set_error(V1C_E_INVALID, me + ": rings must be 8-byte aligned");
    const int maxv = elem_bytes == 1 ? 255 : 65535;
    if (params->rings < kRingsMin || params->rings > kRingsMax || params->r2 < 1 || params->r2 >= ((int64_t)1 << (kR2Bits + 1)) || params->lo < 0 ||
        params->hi > maxv || params->lo > params->hi)
        return set_error(V1C_E_INVALID, me + ": parameter out of range (rings 16..1024, 1 <= r2 < 2^35, 0 <= lo <= hi <= the type's maximum)");
    DeviceGuard dg(device);
    if (!dg.ok)
        return set_error(V1C_E_NODEVICE, "hipSetDevice failed");
    const RingParams prm{params->cx, params->cy, params->r2, params->rings, params->lo, params->hi};
    VIG_HIP_TRY(launch_rings((const uint8_t*)src, src_pitch, h, w, cn, elem_bytes, prm, rings_dev, (hipStream_t)stream));
    return V1C_OK;
}
