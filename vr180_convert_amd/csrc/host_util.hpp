// host_util.hpp -- what the host sides of the C ABI's entry points (plan.hip, feat.hip, png.hip, jpeg.hip, jpegdec.hip, jpegxc.hip,
// jpegxf.hip) share: the error message, the device of a call and the ordinals the decoding entries take, its stream-ordered workspace
// and the alignment of the buffers in it, and whether its stream is being captured.  Host code only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

namespace v1c {

int set_error(int code, const std::string& msg);  // plan.hip: the message v1c_last_error returns

constexpr int kMaxDevices = 64;  // device ordinals the JPEG decoding entries take: one staging buffer each (jpegdec.hip)

// the device of one call; the caller's comes back on every way out
struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) != hipSuccess)
            prev = -1;
        ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard()
    {
        if (prev >= 0)
            (void)hipSetDevice(prev);
    }
};

// the stream-ordered workspace of one call, released on every way out
struct Workspace {
    uint8_t* p = nullptr;
    hipStream_t st;
    explicit Workspace(hipStream_t s) : st(s) {}
    ~Workspace()
    {
        if (p)
            (void)hipFreeAsync(p, st);
    }
};

inline size_t align256(size_t n)
{
    return (n + 255) & ~(size_t)255;
}

// whether work put on `st` now goes into a graph; a stream that cannot be asked counts as not capturing
inline bool stream_is_capturing(hipStream_t st)
{
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone;
}

}  // namespace v1c
