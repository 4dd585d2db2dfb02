// jpeg.hip -- host side of the JPEG entry points of the C ABI (v1c_jpeg_*, include/vr180_remap.h): argument checks, the tables, the
// chain of kernels, and the two copies to the host (the size, then the scan).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/vr180_remap.h"
#include "jpeg_host.hpp"
#include "jpeg_launch.hpp"

namespace v1c {
int set_error(int code, const std::string& msg);  // plan.hip: the message v1c_last_error returns
}

using namespace v1c;
using namespace v1c::jpeg;

namespace {

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

size_t align256(size_t n)
{
    return (n + 255) & ~(size_t)255;
}

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

}  // namespace

extern "C" uint64_t v1c_jpeg_bound(int h, int w, int cn, int subsampling, int restart_mcus)
{
    Geom g;
    return make_geom(h, w, cn, subsampling, restart_mcus, g) ? scan_bound(g) : 0;
}

extern "C" int64_t v1c_jpeg_header(int h, int w, int cn, int quality, int subsampling, int restart_mcus, uint8_t* out, uint64_t capacity)
{
    Geom g;
    if (!out || quality < 1 || quality > 100 || !make_geom(h, w, cn, subsampling, restart_mcus, g))
        return set_error(V1C_E_INVALID, "v1c_jpeg_header: NULL pointer, or cn, quality, subsampling, restart_mcus or sizes out of range");
    const std::vector<uint8_t> head = file_header(g, quality);
    if (capacity < head.size())
        return set_error(V1C_E_INVALID, "v1c_jpeg_header: capacity is below V1C_JPEG_HEADER_MAX");
    std::memcpy(out, head.data(), head.size());
    return (int64_t)head.size();
}

extern "C" int v1c_jpeg_encode(int device, void* stream, const void* img, int h, int w, int64_t pitch, int cn, int quality, int subsampling,
                               int restart_mcus, uint8_t* out_host, uint64_t capacity, uint64_t* size_out)
{
    if (!img || !out_host || !size_out)
        return set_error(V1C_E_INVALID, "v1c_jpeg_encode: NULL pointer");
    if (cn != 1 && cn != 3 && cn != 4)
        return set_error(V1C_E_INVALID, "v1c_jpeg_encode: cn must be 1, 3 or 4");
    if (quality < 1 || quality > 100)
        return set_error(V1C_E_INVALID, "v1c_jpeg_encode: quality must be 1 ... 100");
    if (subsampling != V1C_JPEG_444 && subsampling != V1C_JPEG_420)
        return set_error(V1C_E_INVALID, "v1c_jpeg_encode: subsampling must be V1C_JPEG_444 or V1C_JPEG_420");
    if (restart_mcus < 1 || restart_mcus > 65535)
        return set_error(V1C_E_INVALID, "v1c_jpeg_encode: restart_mcus must be 1 ... 65535");
    Geom g;
    if (!make_geom(h, w, cn, subsampling, restart_mcus, g))
        return set_error(V1C_E_INVALID, "v1c_jpeg_encode: sizes must be 1 ... 65535");
    if (pitch < (int64_t)w * cn)
        return set_error(V1C_E_INVALID, "v1c_jpeg_encode: pitch is smaller than a row's bytes");
    const uint64_t cap = scan_bound(g);
    if (capacity < cap)
        return set_error(V1C_E_INVALID, "v1c_jpeg_encode: capacity " + std::to_string(capacity) + " is below v1c_jpeg_bound = " +
                                            std::to_string(cap));

    DeviceGuard dg(device);
    if (!dg.ok)
        return set_error(V1C_E_NODEVICE, "hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    const uint64_t nraw = raw_bound(g), pieces = nraw / kPiece;
    const uint64_t nsums = std::max<uint64_t>((pieces + kScanChunk - 1) / kScanChunk, ((uint64_t)g.nblocks + kScanChunk - 1) / kScanChunk) + 1;
    const size_t o_tab = 0, o_total = o_tab + align256(sizeof(Tables)), o_coef = o_total + 256;
    const size_t o_bits = o_coef + align256((size_t)g.nblocks * 128), o_bitoff = o_bits + align256((size_t)g.nblocks * 4);
    const size_t o_ibytes = o_bitoff + align256(((size_t)g.nblocks + 1) * 8), o_ioff = o_ibytes + align256((size_t)g.nint * 4);
    const size_t o_raw = o_ioff + align256(((size_t)g.nint + 1) * 8), o_ffcnt = o_raw + align256(nraw + 16);
    const size_t o_ffoff = o_ffcnt + align256(pieces * 4), o_sums = o_ffoff + align256((pieces + 1) * 8);
    const size_t o_out = o_sums + align256(nsums * 8), bytes = o_out + align256(cap + 8);
    Workspace ws(st);
    hipError_t e = hipMallocAsync((void**)&ws.p, bytes, st);
    if (e != hipSuccess)
        return set_error(V1C_E_HIP, std::string("v1c_jpeg_encode: hipMallocAsync: ") + hipGetErrorString(e));
    Args a{};
    a.img = (const uint8_t*)img;
    a.pitch = pitch;
    a.g = g;
    a.tab = (const Tables*)(ws.p + o_tab);
    a.total = (uint64_t*)(ws.p + o_total);
    a.coef = (int16_t*)(ws.p + o_coef);
    a.bits = (uint32_t*)(ws.p + o_bits);
    a.bitoff = (uint64_t*)(ws.p + o_bitoff);
    a.ibytes = (uint32_t*)(ws.p + o_ibytes);
    a.ioff = (uint64_t*)(ws.p + o_ioff);
    a.raw = (uint32_t*)(ws.p + o_raw);
    a.ffcnt = (uint32_t*)(ws.p + o_ffcnt);
    a.ffoff = (uint64_t*)(ws.p + o_ffoff);
    a.sums = (uint64_t*)(ws.p + o_sums);
    a.out = ws.p + o_out;

    Tables tab;  // (pageable: alive until the first synchronisation below, on every way out)
    make_tables(quality, tab);
    uint64_t total = 0;
    e = hipMemcpyAsync(ws.p + o_tab, &tab, sizeof(tab), hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = hipMemsetAsync(a.raw, 0, align256(nraw + 16), st);
    if (e == hipSuccess)
        e = hipMemsetAsync(a.total, 0, 8, st);
    if (e == hipSuccess)
        e = launch_encode(a, st);
    if (e == hipSuccess)
        e = hipMemcpyAsync(&total, a.total, 8, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);  // 1: the size
    if (e == hipSuccess)
        e = es;
    if (e != hipSuccess)
        return set_error(V1C_E_HIP, std::string("v1c_jpeg_encode (kernels): ") + hipGetErrorString(e));
    if (total == 0 || total > cap)
        return set_error(V1C_E_HIP, "v1c_jpeg_encode: internal size estimate exceeded");
    e = hipMemcpyAsync(out_host, a.out, total, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess)
        e = hipStreamSynchronize(st);  // 2: the scan
    if (e != hipSuccess)
        return set_error(V1C_E_HIP, std::string("v1c_jpeg_encode (copy): ") + hipGetErrorString(e));
    *size_out = total;
    return V1C_OK;
}
