// png.hip -- host side of the PNG entry points of the C ABI (v1c_png_*, include/vr180_remap.h): argument checks, pass 1, the codes
// built from its histograms (png_host.hpp), pass 2 and the copy of the stream to the host.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/vr180_remap.h"
#include "host_util.hpp"
#include "png_host.hpp"
#include "png_launch.hpp"

using namespace v1c;
using namespace v1c::png;

extern "C" uint64_t v1c_png_bound(int h, int w, int cn, int depth, int band_rows)
{
    Layout l;
    return make_layout(h, w, cn, depth, band_rows, l) ? bound(l) : 0;
}

extern "C" int v1c_png_deflate(int device, void* stream, const void* img, int h, int w, int64_t pitch, int cn, int depth, int filter,
                               int band_rows, uint8_t* out_host, uint64_t capacity, v1c_png_band* bands_out, int32_t* n_bands_out,
                               uint64_t* size_out)
{
    if (!img || !out_host || !bands_out || !n_bands_out || !size_out)
        return set_error(V1C_E_INVALID, "v1c_png_deflate: NULL pointer");
    if (cn != 1 && cn != 3 && cn != 4)
        return set_error(V1C_E_INVALID, "v1c_png_deflate: cn must be 1, 3 or 4");
    if (depth != V1C_DEPTH_8U && depth != V1C_DEPTH_16U)
        return set_error(V1C_E_INVALID, "v1c_png_deflate: depth must be V1C_DEPTH_8U or V1C_DEPTH_16U");
    if (filter != V1C_PNG_FILTER_UP && filter != V1C_PNG_FILTER_PAETH)
        return set_error(V1C_E_INVALID, "v1c_png_deflate: filter must be 2 (Up) or 4 (Paeth)");
    Layout l;
    if (!make_layout(h, w, cn, depth, band_rows, l))
        return set_error(V1C_E_INVALID, "v1c_png_deflate: sizes must be 1..2^20, band_rows >= 1 and a band below 2^31 scanline bytes");
    if (pitch < (int64_t)l.stride - 1)
        return set_error(V1C_E_INVALID, "v1c_png_deflate: pitch is smaller than a row's bytes");
    if (depth == V1C_DEPTH_16U && (((uintptr_t)img | (uint64_t)pitch) & 1))
        return set_error(V1C_E_INVALID, "v1c_png_deflate: a 16-bit image needs an even pointer and pitch");
    const uint64_t cap = bound(l);
    if (capacity < cap)
        return set_error(V1C_E_INVALID, "v1c_png_deflate: capacity " + std::to_string(capacity) + " is below v1c_png_bound = " +
                                            std::to_string(cap));

    DeviceGuard dg(device);
    if (!dg.ok)
        return set_error(V1C_E_NODEVICE, "hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    const size_t nb = l.n_bands, nseg = nb * l.segs_per_band;
    // the OR list: at most 143 header halfwords (two words each where they straddle) and 4 tail words per coded band, 4 per stored block
    const size_t max_or = nb * 300 + 4 * (size_t)(cap / kStoredMax + nb);
    const size_t o_hist = 0, o_adler = o_hist + align256(nb * kHistStride * 4), o_bands = o_adler + align256(nb * 16);
    const size_t o_tables = o_bands + align256(nb * sizeof(BandDev)), o_segbits = o_tables + align256(nb * kSymbols * 4);
    const size_t o_segoff = o_segbits + align256(nseg * 4), o_or = o_segoff + align256(nseg * 8);
    const size_t o_out = o_or + align256(max_or * sizeof(OrWord)), bytes = o_out + align256(cap + 8);
    Workspace ws(st);
    hipError_t e = hipMallocAsync((void**)&ws.p, bytes, st);
    if (e != hipSuccess)
        return set_error(V1C_E_HIP, std::string("v1c_png_deflate: hipMallocAsync: ") + hipGetErrorString(e));
    Args a{};
    a.img = (const uint8_t*)img;
    a.pitch = pitch;
    a.h = l.h;
    a.stride = l.stride;
    a.filter = filter;
    a.band_rows = l.band_rows;
    a.n_bands = l.n_bands;
    a.segs_per_band = l.segs_per_band;
    a.groups = l.groups;
    a.hist = (uint32_t*)(ws.p + o_hist);
    a.adler = (unsigned long long*)(ws.p + o_adler);
    a.bands = (const BandDev*)(ws.p + o_bands);
    a.tables = (const uint32_t*)(ws.p + o_tables);
    a.segbits = (uint32_t*)(ws.p + o_segbits);
    a.segoff = (uint64_t*)(ws.p + o_segoff);
    a.out = (uint32_t*)(ws.p + o_out);

    // pass 1 and its results (histograms and Adler sums lie next to each other: one copy)
    std::vector<uint8_t> host(o_bands);
    e = hipMemsetAsync(ws.p, 0, o_bands, st);
    if (e == hipSuccess)
        e = launch_pass1(a, l.bpp, st);
    if (e == hipSuccess)
        e = hipMemcpyAsync(host.data(), ws.p, o_bands, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess)
        e = hipMemsetAsync(a.out, 0, align256(cap + 8), st);  // (overlaps the host's work below)
    if (e == hipSuccess)
        e = hipStreamSynchronize(st);
    if (e != hipSuccess)
        return set_error(V1C_E_HIP, std::string("v1c_png_deflate (pass 1): ") + hipGetErrorString(e));

    Plan plan;
    plan_image(l, (const uint32_t*)(host.data() + o_hist), plan);
    if (plan.total > cap || plan.ors.size() > max_or)
        return set_error(V1C_E_HIP, "v1c_png_deflate: internal size estimate exceeded");
    const uint64_t* sums = (const uint64_t*)(host.data() + o_adler);
    for (uint32_t b = 0; b < l.n_bands; b++) {
        v1c_png_band& r = bands_out[b];
        r.row0 = b * l.band_rows;
        r.row1 = std::min(l.h, r.row0 + l.band_rows);
        r.offset = plan.offset[b];
        r.size = plan.bands[b].size;
        r.adler32 = band_adler(sums[2 * b], sums[2 * b + 1], l.band_bytes(b));
        r.stored = plan.bands[b].stored ? 1u : 0u;
    }

    // pass 2
    e = hipMemcpyAsync(ws.p + o_bands, plan.dev.data(), nb * sizeof(BandDev), hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = hipMemcpyAsync(ws.p + o_tables, plan.tables.data(), plan.tables.size() * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && !plan.ors.empty())
        e = hipMemcpyAsync(ws.p + o_or, plan.ors.data(), plan.ors.size() * sizeof(OrWord), hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = launch_pass2(a, l.bpp, plan.any_coded, plan.any_stored, (const OrWord*)(ws.p + o_or), (uint32_t)plan.ors.size(), st);
    if (e == hipSuccess)
        e = hipMemcpyAsync(out_host, a.out, plan.total, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess)
        e = hipStreamSynchronize(st);  // (also keeps `plan`'s pageable buffers alive until their copies are done)
    if (e != hipSuccess)
        return set_error(V1C_E_HIP, std::string("v1c_png_deflate (pass 2): ") + hipGetErrorString(e));
    *n_bands_out = (int32_t)l.n_bands;
    *size_out = plan.total;
    return V1C_OK;
}
