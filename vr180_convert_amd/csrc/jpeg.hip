// jpeg.hip -- host side of the JPEG entry points of the C ABI (v1c_jpeg_*, include/vr180_remap.h): argument checks, the tables, the
// chain of kernels, and the two copies to the host (the size, then the scan).  The optimising entries (v1c_jpeg_*_opt) run the same
// chunks with the tables of jpeg_opt_core.hpp built on the device between two stages; their records come with the sizes.  Where a
// chunk's pieces lie in its workspace, and its end from the sizes on, is jpeg_chunk.hpp's, which the lossless entries share.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/vr180_remap.h"
#include "host_util.hpp"
#include "jpeg_batch.hpp"
#include "jpeg_chunk.hpp"
#include "jpeg_host.hpp"
#include "jpeg_launch.hpp"
#include "jpeg_opt_kernels.hpp"

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

// One image of a list, of either entry: the caller's arguments, whether it builds tables of its own, and where its results go
struct Item {
    const void* img;
    int64_t pitch;
    int quality;
    bool optimize;
    Result to;
};

// One chunk of a batch: images [lo, hi) in one allocation, one upload and one chain of kernels; then all sizes (and the records of the
// optimising images' tables, in the same copy) and synchronisation 1, every image's scan and synchronisation 2.
hipError_t encode_chunk(hipStream_t st, const std::vector<Item>& images, const std::vector<Geom>& geoms, uint32_t lo, uint32_t hi, std::string& what)
{
    const uint32_t n = hi - lo;
    // the chunk's head, uploaded in one copy: descriptors, work lists, one Tables per distinct quality of the images with the Annex K
    // tables and one per optimising image (the quantiser half is the host's, the code half the device overwrites)
    std::vector<int> quality;
    std::vector<uint32_t> tab_of(n);
    std::vector<int32_t> slot_of(n, -1);
    std::vector<OptSlot> slots;
    for (uint32_t f = 0; f < n; f++) {
        if (images[lo + f].optimize)
            continue;
        const auto it = std::find(quality.begin(), quality.end(), images[lo + f].quality);
        tab_of[f] = (uint32_t)(it - quality.begin());
        if (it == quality.end())
            quality.push_back(images[lo + f].quality);
    }
    for (uint32_t f = 0; f < n; f++) {
        if (!images[lo + f].optimize)
            continue;
        slot_of[f] = (int32_t)slots.size();
        tab_of[f] = (uint32_t)quality.size();
        slots.push_back(OptSlot{tab_of[f], geoms[lo + f].nc == 1 ? 2u : 4u});
        quality.push_back(images[lo + f].quality);
    }
    const size_t nslots = slots.size();
    const HeadLayout h = head_layout(n, quality.size(), nslots, false);
    std::vector<uint8_t> up(h.o_sizes, 0);  // (pageable: alive until the first synchronisation of finish_chunk, on every way out)
    Image* im = (Image*)(up.data() + h.o_im);
    uint32_t* first = (uint32_t*)(up.data() + h.o_first);
    for (uint32_t f = 0; f < n; f++) {
        const Item& v = images[lo + f];
        im[f].img = (const uint8_t*)v.img, im[f].pitch = v.pitch, im[f].g = geoms[lo + f], im[f].tab = tab_of[f];
    }
    const Totals t = place_regions(im, n, first);
    for (size_t k = 0; k < quality.size(); k++)
        make_tables(quality[k], ((Tables*)(up.data() + h.o_tabs))[k]);
    stage_slots(up.data(), h, slot_of, slots);

    Workspace ws(st);
    what = "hipMallocAsync";
    const StageLayout sl = stage_layout(h.bytes, t);
    hipError_t e = hipMallocAsync((void**)&ws.p, sl.bytes, st);
    if (e != hipSuccess)
        return e;
    Batch b;
    OptBatch o;
    chunk_args(h, ws.p, n, nslots, t, sl.at(ws.p), b, o);

    e = hipMemcpyAsync(ws.p, up.data(), h.o_sizes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = hipMemsetAsync(b.buf.raw, 0, sl.raw_bytes, st);
    if (e == hipSuccess)
        e = hipMemsetAsync(b.sizes, 0, h.zero_bytes, st);
    if (e == hipSuccess)
        e = nslots ? launch_encode_batch_opt(b, o, first, st) : launch_encode_batch(b, first, st);
    const char* const steps[] = {"", "kernels", "internal size estimate exceeded", "copy"};
    what = steps[finish_chunk(b, h, im, slot_of, [&](uint32_t f) { return images[lo + f].to; }, st, e)];
    return e;
}

// a checked list in chunks under the budget; `name`: the entry, for the messages
int encode_list(int device, void* stream, const std::vector<Item>& items, const std::vector<Geom>& geoms, uint64_t workspace_budget,
                uint32_t* chunks_out, const std::string& name)
{
    DeviceGuard dg(device);
    if (!dg.ok)
        return set_error(V1C_E_NODEVICE, "hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    if (stream_is_capturing(st))
        return set_error(V1C_E_UNSUPPORTED, name + ": the host reads the sizes between the kernels and the copies, so the call cannot be captured into a graph");
    std::vector<uint64_t> bytes, groups;
    for (size_t i = 0; i < items.size(); i++) {
        *items[i].to.size = 0;
        bytes.push_back(workspace_of(geoms[i]) + (items[i].optimize ? sizeof(Tables) + sizeof(Hist) + sizeof(DhtRecord) + sizeof(OptSlot) + 4 + 1280 : 0));
        groups.push_back(most_groups(geoms[i]));
    }
    uint32_t lo = 0, chunk = 0;
    for (uint32_t hi : chunk_ends(bytes, groups, workspace_budget ? workspace_budget : kDefaultBatchWorkspace)) {
        std::string what;
        const hipError_t e = encode_chunk(st, items, geoms, lo, hi, what);
        if (e != hipSuccess)
            return set_error(V1C_E_HIP, name + " (chunk " + std::to_string(chunk) + ", " + what + "): " + hipGetErrorString(e));
        lo = hi, chunk++;
        if (chunks_out)
            *chunks_out = chunk;
    }
    return V1C_OK;
}

// the segments in front of the scan with the DHT body of an optimising encode in place of the Annex K tables'
bool header_with_dht(const Geom& g, int quality, const uint8_t* dht, uint32_t dht_size, std::vector<uint8_t>& out)
{
    if (!whole_tables(dht, dht_size, g.nc))
        return false;
    out = file_header(g, quality, dht, dht_size);
    return true;
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
    const StageLayout sl = stage_layout(head, t);
    Workspace ws(st);
    hipError_t e = hipMallocAsync((void**)&ws.p, sl.bytes, st);
    if (e != hipSuccess)
        return set_error(V1C_E_HIP, std::string("v1c_jpeg_encode: hipMallocAsync: ") + hipGetErrorString(e));
    Args a{};
    a.img = (const uint8_t*)img;
    a.pitch = pitch;
    a.g = g;
    a.tab = (const Tables*)(ws.p + o_tab);
    a.total = (uint64_t*)(ws.p + o_total);
    a.buf = sl.at(ws.p);

    Tables tab;  // (pageable: alive until the first synchronisation below, on every way out)
    make_tables(quality, tab);
    uint64_t total = 0;
    e = hipMemcpyAsync(ws.p + o_tab, &tab, sizeof(tab), hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = hipMemsetAsync(a.buf.raw, 0, sl.raw_bytes, st);
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
    std::vector<Item> items;
    for (int i = 0; i < n; i++)
        items.push_back(Item{images[i].img, images[i].pitch, images[i].quality, false, {images[i].out_host, &images[i].size, nullptr, nullptr}});
    return encode_list(device, stream, items, geoms, workspace_budget, chunks_out, "v1c_jpeg_encode_batch");
}

extern "C" int64_t v1c_jpeg_header_opt(int h, int w, int cn, int quality, int subsampling, int restart_mcus, const uint8_t* dht, uint32_t dht_size,
                                       uint8_t* out, uint64_t capacity)
{
    Geom g;
    if (!out || !dht || quality < 1 || quality > 100 || !make_geom(h, w, cn, subsampling, restart_mcus, g))
        return set_error(V1C_E_INVALID, "v1c_jpeg_header_opt: NULL pointer, or cn, quality, subsampling, restart_mcus or sizes out of range");
    std::vector<uint8_t> head;
    if (dht_size > V1C_JPEG_DHT_MAX || !header_with_dht(g, quality, dht, dht_size, head))
        return set_error(V1C_E_INVALID, "v1c_jpeg_header_opt: dht is not the tables of an optimising encode of such an image");
    if (capacity < head.size())
        return set_error(V1C_E_INVALID, "v1c_jpeg_header_opt: capacity is below V1C_JPEG_HEADER_OPT_MAX");
    std::memcpy(out, head.data(), head.size());
    return (int64_t)head.size();
}

extern "C" int v1c_jpeg_encode_opt(int device, void* stream, const void* img, int h, int w, int64_t pitch, int cn, int quality, int subsampling,
                                   int restart_mcus, uint8_t* out_host, uint64_t capacity, uint64_t* size_out, uint8_t* dht_out,
                                   uint32_t* dht_size_out)
{
    if (!size_out || !dht_out || !dht_size_out)
        return set_error(V1C_E_INVALID, "v1c_jpeg_encode_opt: NULL pointer");
    std::vector<Geom> geoms(1);
    const std::string bad = image_error(img, h, w, pitch, cn, quality, subsampling, restart_mcus, out_host, capacity, geoms[0]);
    if (!bad.empty())
        return set_error(V1C_E_INVALID, "v1c_jpeg_encode_opt: " + bad);
    *dht_size_out = 0;
    const std::vector<Item> items = {Item{img, pitch, quality, true, {out_host, size_out, dht_out, dht_size_out}}};
    return encode_list(device, stream, items, geoms, 0, nullptr, "v1c_jpeg_encode_opt");
}

extern "C" int v1c_jpeg_encode_batch_opt(int device, void* stream, int n, v1c_jpeg_image_opt* images, uint64_t workspace_budget, uint32_t* chunks_out)
{
    if (chunks_out)
        *chunks_out = 0;
    if (n < 0)
        return set_error(V1C_E_INVALID, "v1c_jpeg_encode_batch_opt: n is negative");
    if (n == 0)
        return V1C_OK;
    if (!images)
        return set_error(V1C_E_INVALID, "v1c_jpeg_encode_batch_opt: NULL pointer");
    std::vector<Geom> geoms((size_t)n);
    std::vector<Item> items;
    for (int i = 0; i < n; i++) {
        v1c_jpeg_image_opt& v = images[i];
        const std::string bad = image_error(v.img, v.h, v.w, v.pitch, v.cn, v.quality, v.subsampling, v.restart_mcus, v.out_host, v.capacity, geoms[i]);
        if (!bad.empty())
            return set_error(V1C_E_INVALID, "v1c_jpeg_encode_batch_opt: image " + std::to_string(i) + ": " + bad);
        v.dht_size = 0;
        items.push_back(Item{v.img, v.pitch, v.quality, v.optimize != 0, {v.out_host, &v.size, v.dht, &v.dht_size}});
    }
    return encode_list(device, stream, items, geoms, workspace_budget, chunks_out, "v1c_jpeg_encode_batch_opt");
}
