// jpeg.hip -- host side of the JPEG entry points of the C ABI (v1c_jpeg_*, include/vr180_remap.h): argument checks, the tables, the
// chain of kernels, and the two copies to the host (the size, then the scan).  The optimising entries (v1c_jpeg_*_opt) run the same
// chunks with the tables of jpeg_opt_core.hpp built on the device between two stages; their records come with the sizes.
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

// One image of a list, of either entry: the caller's arguments, where its results go, and whether it builds tables of its own
struct Item {
    const void* img;
    int64_t pitch;
    int quality;
    uint8_t* out_host;
    uint64_t* size;
    bool optimize;
    uint8_t* dht;        // optimising images: V1C_JPEG_DHT_MAX bytes for the DHT segment's body
    uint32_t* dht_size;
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
    const size_t o_im = 0, o_first = o_im + align256((size_t)n * sizeof(Image)), o_tabs = o_first + align256((size_t)kWorkLists * (n + 1) * 4);
    const size_t o_slotof = o_tabs + align256(quality.size() * sizeof(Tables));
    const size_t o_slots = o_slotof + (nslots ? align256((size_t)n * 4) : 0), o_sizes = o_slots + align256(nslots * sizeof(OptSlot));
    // read back in one copy: the sizes, then the records; zeroed with them: the histograms
    const size_t o_rec = o_sizes + align256((size_t)n * 8), o_hist = o_rec + align256(nslots * sizeof(DhtRecord));
    const size_t head = o_hist + align256(nslots * sizeof(Hist));
    const size_t back_bytes = nslots ? o_rec + nslots * sizeof(DhtRecord) - o_sizes : (size_t)n * 8;
    std::vector<uint8_t> up(o_sizes, 0);  // (pageable: alive until the first synchronisation below, on every way out)
    Image* im = (Image*)(up.data() + o_im);
    uint32_t* first = (uint32_t*)(up.data() + o_first);
    for (uint32_t f = 0; f < n; f++) {
        const Item& v = images[lo + f];
        im[f].img = (const uint8_t*)v.img, im[f].pitch = v.pitch, im[f].g = geoms[lo + f], im[f].tab = tab_of[f];
    }
    const Totals t = place_regions(im, n, first);
    for (size_t k = 0; k < quality.size(); k++)
        make_tables(quality[k], ((Tables*)(up.data() + o_tabs))[k]);
    if (nslots) {
        std::memcpy(up.data() + o_slotof, slot_of.data(), (size_t)n * 4);
        std::memcpy(up.data() + o_slots, slots.data(), nslots * sizeof(OptSlot));
    }

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
    OptBatch o{};
    o.slot_of = (const int32_t*)(ws.p + o_slotof), o.slots = (const OptSlot*)(ws.p + o_slots), o.nslots = (uint32_t)nslots;
    o.hist = (Hist*)(ws.p + o_hist), o.rec = (DhtRecord*)(ws.p + o_rec), o.tabs = (Tables*)(ws.p + o_tabs);

    what = "kernels";
    std::vector<uint8_t> back(back_bytes, 0);
    e = hipMemcpyAsync(ws.p, up.data(), o_sizes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = hipMemsetAsync(b.buf.raw, 0, bs.raw_bytes, st);
    if (e == hipSuccess)
        e = hipMemsetAsync(b.sizes, 0, nslots ? head - o_sizes : (size_t)n * 8, st);
    if (e == hipSuccess)
        e = nslots ? launch_encode_batch_opt(b, o, first, st) : launch_encode_batch(b, first, st);
    if (e == hipSuccess)
        e = hipMemcpyAsync(back.data(), b.sizes, back_bytes, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);  // 1: the sizes and the records
    if (e == hipSuccess)
        e = es;
    if (e != hipSuccess)
        return e;
    const uint64_t* sizes = (const uint64_t*)back.data();
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
    for (uint32_t f = 0; f < n; f++) {
        *images[lo + f].size = sizes[f];
        if (slot_of[f] >= 0)
            *images[lo + f].dht_size = dht_body(((const DhtRecord*)(back.data() + (o_rec - o_sizes)))[slot_of[f]], images[lo + f].dht);
    }
    return hipSuccess;
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
        *items[i].size = 0;
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
    // the body must be whole tables: the two of one component, or the four of three, in the segment's order
    const uint8_t ids[4] = {0x00, 0x10, 0x01, 0x11};
    uint32_t at = 0, tables = 0;
    while (at < dht_size && tables < 4) {
        if (dht[at] != ids[tables] || at + 17 > dht_size)
            return false;
        uint32_t nsym = 0;
        for (int i = 0; i < 16; i++)
            nsym += dht[at + 1 + i];
        if (nsym < 1 || nsym > 256)
            return false;
        at += 17 + nsym, tables++;
    }
    if (at != dht_size || tables != (g.nc == 1 ? 2u : 4u))
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
    std::vector<Item> items;
    for (int i = 0; i < n; i++)
        items.push_back(Item{images[i].img, images[i].pitch, images[i].quality, images[i].out_host, &images[i].size, false, nullptr, nullptr});
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
    const std::vector<Item> items = {Item{img, pitch, quality, out_host, size_out, true, dht_out, dht_size_out}};
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
        items.push_back(Item{v.img, v.pitch, v.quality, v.out_host, &v.size, v.optimize != 0, v.dht, &v.dht_size});
    }
    return encode_list(device, stream, items, geoms, workspace_budget, chunks_out, "v1c_jpeg_encode_batch_opt");
}
