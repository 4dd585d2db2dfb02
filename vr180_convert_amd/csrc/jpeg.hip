// jpeg.hip -- host side of the JPEG entry points of the C ABI (v1c_jpeg_*, include/vr180_remap.h): argument checks, the tables, the
// chain of kernels, and the two copies to the host (the size, then the scan).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/vr180_remap.h"
#include "host_util.hpp"
#include "jpeg_batch.hpp"
#include "jpeg_host.hpp"
#include "jpeg_launch.hpp"

using namespace v1c;
using namespace v1c::jpeg;

namespace {

// the argument rules of one image, for the single call and for every image of a batch: what is wrong, or nothing; g: its geometry
std::string image_error(const void* img, int h, int w, int64_t pitch, int cn, int quality, int subsampling, int restart_mcus,
                        const uint8_t* out_host, uint64_t capacity, Geom& g)
{
    if (!img || !out_host)
        return "NULL pointer";
    if (cn != 1 && cn != 3 && cn != 4)
        return "cn must be 1, 3 or 4";
    if (quality < 1 || quality > 100)
        return "quality must be 1 ... 100";
    if (subsampling != V1C_JPEG_444 && subsampling != V1C_JPEG_420)
        return "subsampling must be V1C_JPEG_444 or V1C_JPEG_420";
    if (restart_mcus < 1 || restart_mcus > 65535)
        return "restart_mcus must be 1 ... 65535";
    if (!make_geom(h, w, cn, subsampling, restart_mcus, g))
        return "sizes must be 1 ... 65535";
    if (pitch < (int64_t)w * cn)
        return "pitch is smaller than a row's bytes";
    if (capacity < scan_bound(g))
        return "capacity " + std::to_string(capacity) + " is below v1c_jpeg_bound = " + std::to_string(scan_bound(g));
    return std::string();
}

// The workspace of a call on ws: the `head` bytes the call lays out itself, and behind them the encoder's buffers for `t` entries back to
// back, each aligned to 256 bytes.
struct BufferSet {
    Buffers buf;
    size_t raw_bytes;  // of buf.raw, to be zeroed
    size_t bytes;      // of the workspace, head included
};

hipError_t allocate_buffers(Workspace& ws, size_t head, const Totals& t, BufferSet& s)
{
    s.raw_bytes = align256(t.pieces * kPiece + 16);
    const size_t o_coef = head, o_bits = o_coef + align256(t.nblocks * 128), o_bitoff = o_bits + align256(t.nblocks * 4);
    const size_t o_ibytes = o_bitoff + align256((t.nblocks + 1) * 8), o_ioff = o_ibytes + align256(t.nint * 4);
    const size_t o_raw = o_ioff + align256((t.nint + 1) * 8), o_ffcnt = o_raw + s.raw_bytes, o_ffoff = o_ffcnt + align256(t.pieces * 4);
    const size_t o_sums = o_ffoff + align256((t.pieces + 1) * 8), o_out = o_sums + align256(sums_of(t, kScanChunk) * 8);
    s.bytes = o_out + align256(t.out_bytes + 8);
    const hipError_t e = hipMallocAsync((void**)&ws.p, s.bytes, ws.st);
    if (e != hipSuccess)
        return e;
    uint8_t* base = ws.p;
    s.buf.coef = (int16_t*)(base + o_coef);
    s.buf.bits = (uint32_t*)(base + o_bits);
    s.buf.bitoff = (uint64_t*)(base + o_bitoff);
    s.buf.ibytes = (uint32_t*)(base + o_ibytes);
    s.buf.ioff = (uint64_t*)(base + o_ioff);
    s.buf.raw = (uint32_t*)(base + o_raw);
    s.buf.ffcnt = (uint32_t*)(base + o_ffcnt);
    s.buf.ffoff = (uint64_t*)(base + o_ffoff);
    s.buf.sums = (uint64_t*)(base + o_sums);
    s.buf.out = base + o_out;
    return hipSuccess;
}

// One chunk of a batch: images [lo, hi) in one allocation, one upload and one chain of kernels; then all sizes and synchronisation 1,
// every image's scan and synchronisation 2.
hipError_t encode_chunk(hipStream_t st, v1c_jpeg_image* images, const std::vector<Geom>& geoms, uint32_t lo, uint32_t hi, std::string& what)
{
    const uint32_t n = hi - lo;
    // the chunk's head, uploaded in one copy: descriptors, work lists, one Tables per distinct quality
    std::vector<int> quality;
    std::vector<uint32_t> tab_of(n);
    for (uint32_t f = 0; f < n; f++) {
        const auto it = std::find(quality.begin(), quality.end(), images[lo + f].quality);
        tab_of[f] = (uint32_t)(it - quality.begin());
        if (it == quality.end())
            quality.push_back(images[lo + f].quality);
    }
    const size_t o_im = 0, o_first = o_im + align256((size_t)n * sizeof(Image)), o_tabs = o_first + align256((size_t)kWorkLists * (n + 1) * 4);
    const size_t o_sizes = o_tabs + align256(quality.size() * sizeof(Tables)), head = o_sizes + align256((size_t)n * 8);
    std::vector<uint8_t> up(o_sizes, 0);  // (pageable: alive until the first synchronisation below, on every way out)
    Image* im = (Image*)(up.data() + o_im);
    uint32_t* first = (uint32_t*)(up.data() + o_first);
    for (uint32_t f = 0; f < n; f++) {
        const v1c_jpeg_image& v = images[lo + f];
        im[f].img = (const uint8_t*)v.img, im[f].pitch = v.pitch, im[f].g = geoms[lo + f], im[f].tab = tab_of[f];
    }
    const Totals t = place_regions(im, n, first);
    for (size_t k = 0; k < quality.size(); k++)
        make_tables(quality[k], ((Tables*)(up.data() + o_tabs))[k]);

    Workspace ws(st);
    what = "hipMallocAsync";
    BufferSet bs;
    hipError_t e = allocate_buffers(ws, head, t, bs);
    if (e != hipSuccess)
        return e;
    Batch b{};
    b.im = (const Image*)(ws.p + o_im), b.first = (const uint32_t*)(ws.p + o_first), b.tabs = (const Tables*)(ws.p + o_tabs);
    b.n = n, b.t = t;
    b.sizes = (uint64_t*)(ws.p + o_sizes);
    b.buf = bs.buf;

    what = "kernels";
    std::vector<uint64_t> sizes(n, 0);
    e = hipMemcpyAsync(ws.p, up.data(), o_sizes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = hipMemsetAsync(b.buf.raw, 0, bs.raw_bytes, st);
    if (e == hipSuccess)
        e = hipMemsetAsync(b.sizes, 0, (size_t)n * 8, st);
    if (e == hipSuccess)
        e = launch_encode_batch(b, first, st);
    if (e == hipSuccess)
        e = hipMemcpyAsync(sizes.data(), b.sizes, (size_t)n * 8, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);  // 1: the sizes
    if (e == hipSuccess)
        e = es;
    if (e != hipSuccess)
        return e;
    what = "internal size estimate exceeded";
    for (uint32_t f = 0; f < n; f++)
        if (sizes[f] == 0 || sizes[f] > scan_bound(im[f].g))
            return hipErrorUnknown;
    what = "copy";
    for (uint32_t f = 0; f < n && e == hipSuccess; f++)
        e = hipMemcpyAsync(images[lo + f].out_host, b.buf.out + im[f].out0, sizes[f], hipMemcpyDeviceToHost, st);
    const hipError_t ec = hipStreamSynchronize(st);  // 2: the scans
    if (e == hipSuccess)
        e = ec;
    if (e != hipSuccess)
        return e;
    for (uint32_t f = 0; f < n; f++)
        images[lo + f].size = sizes[f];
    return hipSuccess;
}

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
    if (!size_out)
        return set_error(V1C_E_INVALID, "v1c_jpeg_encode: NULL pointer");
    Geom g;
    const std::string bad = image_error(img, h, w, pitch, cn, quality, subsampling, restart_mcus, out_host, capacity, g);
    if (!bad.empty())
        return set_error(V1C_E_INVALID, "v1c_jpeg_encode: " + bad);
    const uint64_t cap = scan_bound(g);

    DeviceGuard dg(device);
    if (!dg.ok)
        return set_error(V1C_E_NODEVICE, "hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    const Totals t{g.nblocks, g.nint, pieces_of(g), cap};
    const size_t o_tab = 0, o_total = o_tab + align256(sizeof(Tables)), head = o_total + 256;
    Workspace ws(st);
    BufferSet bs;
    hipError_t e = allocate_buffers(ws, head, t, bs);
    if (e != hipSuccess)
        return set_error(V1C_E_HIP, std::string("v1c_jpeg_encode: hipMallocAsync: ") + hipGetErrorString(e));
    Args a{};
    a.img = (const uint8_t*)img;
    a.pitch = pitch;
    a.g = g;
    a.tab = (const Tables*)(ws.p + o_tab);
    a.total = (uint64_t*)(ws.p + o_total);
    a.buf = bs.buf;

    Tables tab;  // (pageable: alive until the first synchronisation below, on every way out)
    make_tables(quality, tab);
    uint64_t total = 0;
    e = hipMemcpyAsync(ws.p + o_tab, &tab, sizeof(tab), hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = hipMemsetAsync(a.buf.raw, 0, bs.raw_bytes, st);
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
    e = hipMemcpyAsync(out_host, a.buf.out, total, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess)
        e = hipStreamSynchronize(st);  // 2: the scan
    if (e != hipSuccess)
        return set_error(V1C_E_HIP, std::string("v1c_jpeg_encode (copy): ") + hipGetErrorString(e));
    *size_out = total;
    return V1C_OK;
}

extern "C" int v1c_jpeg_encode_batch(int device, void* stream, int n, v1c_jpeg_image* images, uint64_t workspace_budget, uint32_t* chunks_out)
{
    if (chunks_out)
        *chunks_out = 0;
    if (n < 0)
        return set_error(V1C_E_INVALID, "v1c_jpeg_encode_batch: n is negative");
    if (n == 0)
        return V1C_OK;
    if (!images)
        return set_error(V1C_E_INVALID, "v1c_jpeg_encode_batch: NULL pointer");
    // every image's arguments before any device call: all or nothing
    std::vector<Geom> geoms((size_t)n);
    for (int i = 0; i < n; i++) {
        const v1c_jpeg_image& v = images[i];
        const std::string bad = image_error(v.img, v.h, v.w, v.pitch, v.cn, v.quality, v.subsampling, v.restart_mcus, v.out_host, v.capacity, geoms[i]);
        if (!bad.empty())
            return set_error(V1C_E_INVALID, "v1c_jpeg_encode_batch: image " + std::to_string(i) + ": " + bad);
    }
    DeviceGuard dg(device);
    if (!dg.ok)
        return set_error(V1C_E_NODEVICE, "hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    if (stream_is_capturing(st))
        return set_error(V1C_E_UNSUPPORTED, "v1c_jpeg_encode_batch: the host reads the sizes between the kernels and the copies, so the call cannot be captured into a graph");
    std::vector<uint64_t> bytes, groups;
    for (int i = 0; i < n; i++) {
        images[i].size = 0;
        bytes.push_back(workspace_of(geoms[i]));
        groups.push_back(most_groups(geoms[i]));
    }
    uint32_t lo = 0, chunk = 0;
    for (uint32_t hi : chunk_ends(bytes, groups, workspace_budget ? workspace_budget : kDefaultBatchWorkspace)) {
        std::string what;
        const hipError_t e = encode_chunk(st, images, geoms, lo, hi, what);
        if (e != hipSuccess)
            return set_error(V1C_E_HIP, "v1c_jpeg_encode_batch (chunk " + std::to_string(chunk) + ", " + what + "): " + hipGetErrorString(e));
        lo = hi, chunk++;
        if (chunks_out)
            *chunks_out = chunk;
    }
    return V1C_OK;
}
