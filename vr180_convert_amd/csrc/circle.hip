// circle.hip -- host side of the image-circle entry points of the C ABI (v1c_fit_circle*, include/vr180_remap.h): argument checks, the
// defaults, the launches of kernels_circle.hip and, for the synchronous form, the copy back and the compaction of the rim points.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/vr180_remap.h"
#include "circle_launch.hpp"
#include "host_util.hpp"

using namespace v1c;
using namespace v1c::circle;

#define CIRCLE_HIP_TRY(expr)                                                                            \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess)                                                                           \
            return set_error(V1C_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));             \
    } while (0)

namespace {

// NULL: threshold 10, runs of 4, four refits within 8, 3, 1.5 and 1.5 px, at least 8 points (DESIGN.md section 21 has the evidence)
const Params kDefaults = {10, 4, 4, 8, {128, 48, 24, 24, 24, 24, 24, 24}};

int check(const char* who, const void* img, int h, int w, int64_t pitch, int cn, int depth, const v1c_circle_params* p, const void* ws,
          const void* out, Params* prm)
{
    const std::string me(who);
    if (!img || !ws || !out)
        return set_error(V1C_E_INVALID, me + ": NULL pointer");
    if (cn != 1 && cn != 3 && cn != 4)
        return set_error(V1C_E_INVALID, me + ": cn must be 1, 3 or 4");
    if (depth != V1C_DEPTH_8U && depth != V1C_DEPTH_16U)
        return set_error(V1C_E_INVALID, me + ": depth must be V1C_DEPTH_8U or V1C_DEPTH_16U");
    const int es = depth == V1C_DEPTH_16U ? 2 : 1;
    if (h <= 0 || w <= 0 || h > 32768 || w > 32768 || pitch < (int64_t)w * cn * es)
        return set_error(V1C_E_INVALID, me + ": image size must be 1..32768 with pitch >= the bytes of a row");
    if (es == 2 && (((uintptr_t)img | (uint64_t)pitch) & 1))
        return set_error(V1C_E_INVALID, me + ": a 16-bit image needs an even pointer and pitch");
    if (((uintptr_t)ws & 3) || ((uintptr_t)out & 7))
        return set_error(V1C_E_INVALID, me + ": workspace must be 4-byte and the result 8-byte aligned");
    *prm = kDefaults;
    if (p) {
        if (p->threshold < 0 || p->threshold > 65535 || p->run < 1 || p->run > kMaxRun || p->rounds < 0 || p->rounds > kMaxRounds ||
            p->min_points < 3 || p->min_points > (1 << 20))
            return set_error(V1C_E_INVALID, me + ": parameter out of range (threshold 0..65535, run 1..64, rounds 0..8, min_points 3..2^20)");
        for (int k = 0; k < p->rounds; k++)
            if (p->tol16[k] < 1 || p->tol16[k] > (1 << 20))
                return set_error(V1C_E_INVALID, me + ": tol16 must be 1..2^20");
        prm->threshold = p->threshold;
        prm->run = p->run;
        prm->rounds = p->rounds;
        prm->min_points = p->min_points;
        for (int k = 0; k < kMaxRounds; k++)
            prm->tol16[k] = k < p->rounds ? p->tol16[k] : 0;
    }
    return V1C_OK;
}

}  // namespace

extern "C" uint64_t v1c_fit_circle_workspace(int h, int w)
{
    if (h <= 0 || w <= 0 || h > 32768 || w > 32768)
        return 0;
    return workspace_bytes(h, w);
}

extern "C" int v1c_fit_circle_async(int device, void* stream, const void* img, int h, int w, int64_t pitch, int cn, int depth,
                                    const v1c_circle_params* params, void* workspace, double* out_dev8)
{
    Params prm;
    int rc = check("v1c_fit_circle_async", img, h, w, pitch, cn, depth, params, workspace, out_dev8, &prm);
    if (rc)
        return rc;
    DeviceGuard dg(device);
    if (!dg.ok)
        return set_error(V1C_E_NODEVICE, "hipSetDevice failed");
    CIRCLE_HIP_TRY(launch_fit((const uint8_t*)img, h, w, pitch, cn, depth == V1C_DEPTH_16U, prm, (uint8_t*)workspace, out_dev8, (hipStream_t)stream));
    return V1C_OK;
}

extern "C" int v1c_fit_circle(int device, void* stream, const void* img, int h, int w, int64_t pitch, int cn, int depth,
                              const v1c_circle_params* params, void* workspace, double* out_host8, v1c_circle_point* points_out,
                              int32_t capacity, int32_t* n_points_out)
{
    Params prm;
    int rc = check("v1c_fit_circle", img, h, w, pitch, cn, depth, params, workspace, out_host8, &prm);
    if (rc)
        return rc;
    if (points_out && (capacity < 0 || !n_points_out))
        return set_error(V1C_E_INVALID, "v1c_fit_circle: points_out needs a capacity >= 0 and n_points_out");
    DeviceGuard dg(device);
    if (!dg.ok)
        return set_error(V1C_E_NODEVICE, "hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    if (stream_is_capturing(st))
        return set_error(V1C_E_UNSUPPORTED, "v1c_fit_circle synchronises: use v1c_fit_circle_async under stream capture");
    uint8_t* ws = (uint8_t*)workspace;
    const size_t ro = result_offset(h, w);
    CIRCLE_HIP_TRY(launch_fit((const uint8_t*)img, h, w, pitch, cn, depth == V1C_DEPTH_16U, prm, ws, (double*)(ws + ro), st));
    std::vector<uint8_t> host(points_out ? ro : 0);
    if (points_out)
        CIRCLE_HIP_TRY(hipMemcpyAsync(host.data(), ws, ro, hipMemcpyDeviceToHost, st));
    CIRCLE_HIP_TRY(hipMemcpyAsync(out_host8, ws + ro, 8 * sizeof(double), hipMemcpyDeviceToHost, st));
    CIRCLE_HIP_TRY(hipStreamSynchronize(st));
    if (points_out) {
        const uint32_t* pts = (const uint32_t*)host.data();
        const uint8_t* sel = host.data() + flags_offset(h, w);
        const size_t n = slots(h, w);
        int64_t m = 0;
        for (size_t i = 0; i < n; i++) {
            if (pts[i] == kNoPoint)
                continue;
            if (m < capacity) {
                points_out[m].x = (int32_t)(pts[i] & 0xFFFFu);
                points_out[m].y = (int32_t)(pts[i] >> 16);
                points_out[m].selected = sel[i];
            }
            m++;
        }
        *n_points_out = (int32_t)m;
        if (m > capacity)
            return set_error(V1C_E_INVALID, "v1c_fit_circle: " + std::to_string(m) + " rim points, capacity " + std::to_string(capacity));
    }
    return V1C_OK;
}
