// jpegdec.hip -- host side of the JPEG decoding entry points of the C ABI (v1c_jpeg_decode*, include/vr180_remap.h): the parse, the
// upload from the page-locked staging buffer, the chain of kernels and the rounds of the synchronisation, whose flag the host reads.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/vr180_remap.h"
#include "jpegdec_host.hpp"
#include "jpegdec_launch.hpp"

namespace v1c {
int set_error(int code, const std::string& msg);  // plan.hip: the message v1c_last_error returns
}

using namespace v1c;
using namespace v1c::jpegdec;

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

// The page-locked staging buffers, one per device, grown on demand and kept: what is uploaded (tables, segment offsets, the scan) and
// the word that comes back.  Each has a lock of its own, held by a call from filling the buffer to its last synchronisation, so the
// buffer is never rewritten under a copy in flight: decodes on ONE device take turns (whatever their streams), decodes on different
// devices do not meet.
constexpr int kMaxDevices = 64;
struct Staging {
    std::mutex mu;
    uint8_t* p = nullptr;
    size_t size = 0;
};
Staging g_staging[kMaxDevices];

// (with s.mu held)
uint8_t* staging(Staging& s, size_t bytes)
{
    if (s.size < bytes) {
        if (s.p)
            (void)hipHostFree(s.p);
        s.p = nullptr, s.size = 0;
        const size_t want = std::max(bytes + bytes / 4, (size_t)1 << 20);
        if (hipHostMalloc((void**)&s.p, want, hipHostMallocDefault) != hipSuccess)
            return nullptr;
        s.size = want;
    }
    return s.p;
}

int parse_error(const char* who, ParseResult r, const Parsed& p, v1c_jpeg_decode_report* report)
{
    if (report)
        report->error_pos = p.error_pos;
    return set_error(r == kUnsupported ? V1C_E_UNSUPPORTED : V1C_E_CORRUPT,
                     std::string(who) + ": " + p.why + " (byte " + std::to_string(p.error_pos) + ")");
}

}  // namespace

extern "C" int v1c_jpeg_decode_info(const uint8_t* file, uint64_t size, v1c_jpeg_info* info)
{
    if (!file || !info)
        return set_error(V1C_E_INVALID, "v1c_jpeg_decode_info: NULL pointer");
    Parsed p;
    const ParseResult r = parse(file, size, p);
    if (r != kParsed)
        return parse_error("v1c_jpeg_decode_info", r, p, nullptr);
    info->height = (int32_t)p.g.h, info->width = (int32_t)p.g.w, info->components = (int32_t)p.g.nc;
    info->h_samp = (int32_t)p.g.hs, info->v_samp = (int32_t)p.g.vs, info->restart_interval = (int32_t)p.restart;
    return V1C_OK;
}

extern "C" int v1c_jpeg_decode(int device, void* stream, const uint8_t* file, uint64_t size, void* out, int64_t pitch, int out_cn,
                               uint32_t subseq_bits, v1c_jpeg_decode_report* report)
{
    if (report)
        std::memset(report, 0, sizeof(*report));
    if (!file || !out)
        return set_error(V1C_E_INVALID, "v1c_jpeg_decode: NULL pointer");
    if (out_cn != 1 && out_cn != 3)
        return set_error(V1C_E_INVALID, "v1c_jpeg_decode: out_cn must be 1 or 3");
    const uint32_t S = subseq_bits ? subseq_bits : kDefaultSubseqBits;
    if (S % 32 || S < 256 || S > (1u << 24))
        return set_error(V1C_E_INVALID, "v1c_jpeg_decode: subseq_bits must be a multiple of 32 from 256 to 2^24, or 0");
    Parsed ps;
    const ParseResult pr = parse(file, size, ps);
    if (pr != kParsed)
        return parse_error("v1c_jpeg_decode", pr, ps, report);
    const Geom& g = ps.g;
    if (out_cn == 1 && g.nc != 1)
        return set_error(V1C_E_INVALID, "v1c_jpeg_decode: out_cn 1 takes a file of one component");
    if (pitch < (int64_t)g.w * out_cn)
        return set_error(V1C_E_INVALID, "v1c_jpeg_decode: pitch is smaller than a row's bytes");

    if (device < 0 || device >= kMaxDevices)
        return set_error(V1C_E_NODEVICE, "v1c_jpeg_decode: no such device");
    DeviceGuard dg(device);
    if (!dg.ok)
        return set_error(V1C_E_NODEVICE, "hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
        return set_error(V1C_E_UNSUPPORTED, "v1c_jpeg_decode: the host reads a flag between the rounds, so the call cannot be captured into a graph");

    const std::vector<uint32_t> subfirst = sub_first(ps, S);
    const uint32_t nseg = g.nseg, nsub = subfirst.back(), nu = ps.segoff.back();
    const uint32_t scan_len = (uint32_t)ps.scan_len, pieces = (scan_len + kPiece - 1) / kPiece;
    if (report)
        report->segments = nseg, report->subsequences = nsub;

    // what is uploaded, back to back in the staging buffer and in the workspace: tables, segment offsets, first subsequences, the scan
    const size_t o_tab = 0, o_segoff = o_tab + align256(sizeof(Tables)), o_subfirst = o_segoff + align256(((size_t)nseg + 1) * 4);
    const size_t o_scan = o_subfirst + align256(((size_t)nseg + 1) * 4), up_bytes = o_scan + align256(((size_t)pieces + 1) * kPiece);
    // ... and what the kernels make
    const uint64_t nmax = std::max<uint64_t>(std::max<uint64_t>(pieces, nsub), g.nblocks);
    const size_t o_flags = up_bytes, o_drop = o_flags + 256, o_dropoff = o_drop + align256((size_t)pieces * 4);
    const size_t o_u = o_dropoff + align256(((size_t)pieces + 1) * 8), u_bytes = align256((size_t)nu + 16);
    const size_t o_exit0 = o_u + u_bytes, o_exit1 = o_exit0 + align256((size_t)nsub * 8), o_last = o_exit1 + align256((size_t)nsub * 8);
    const size_t o_count = o_last + align256((size_t)nsub * 8), o_first = o_count + align256((size_t)nsub * 4);
    const size_t o_coef = o_first + align256(((size_t)nsub + 1) * 8), coef_bytes = align256((size_t)g.nblocks * 128);
    const size_t o_dcd = o_coef + coef_bytes, o_dcoff = o_dcd + align256((size_t)g.nblocks * 4);
    const size_t o_sums = o_dcoff + align256(((size_t)g.nblocks + 1) * 8);
    const size_t o_p0 = o_sums + align256((nmax / jpeg::kScanChunk + 2) * 8);
    const size_t p0_bytes = align256((size_t)plane_pitch(g, 0) * plane_rows(g, 0)), pc_bytes = align256((size_t)plane_pitch(g, 1) * plane_rows(g, 1));
    const size_t bytes = o_p0 + p0_bytes + (g.nc == 3 ? 2 * pc_bytes : 0);

    Staging& sg = g_staging[device];
    std::lock_guard<std::mutex> lock(sg.mu);
    uint8_t* stage = staging(sg, up_bytes + 64);
    if (!stage)
        return set_error(V1C_E_HIP, "v1c_jpeg_decode: hipHostMalloc of the staging buffer failed");
    std::memset(stage, 0, up_bytes);
    std::memcpy(stage + o_tab, &ps.tab, sizeof(Tables));
    std::memcpy(stage + o_segoff, ps.segoff.data(), ((size_t)nseg + 1) * 4);
    std::memcpy(stage + o_subfirst, subfirst.data(), ((size_t)nseg + 1) * 4);
    std::memcpy(stage + o_scan, file + ps.scan_start, (size_t)scan_len + 2);  // (the parse saw the two bytes of the marker behind the scan)
    volatile uint32_t* back = (volatile uint32_t*)(stage + up_bytes);        // what comes back: a round's flag, the verdict

    Workspace ws(st);
    hipError_t e = hipMallocAsync((void**)&ws.p, bytes, st);
    if (e != hipSuccess)
        return set_error(V1C_E_HIP, std::string("v1c_jpeg_decode: hipMallocAsync: ") + hipGetErrorString(e));
    Args a{};
    a.g = g;
    a.tab = (const Tables*)(ws.p + o_tab);
    a.scan = ws.p + o_scan;
    a.scan_len = scan_len, a.pieces = pieces;
    a.drop = (uint32_t*)(ws.p + o_drop);
    a.dropoff = (uint64_t*)(ws.p + o_dropoff);
    a.u = (uint32_t*)(ws.p + o_u);
    a.segoff = (const uint32_t*)(ws.p + o_segoff);
    a.subfirst = (const uint32_t*)(ws.p + o_subfirst);
    a.nsub = nsub, a.S = S;
    a.exit[0] = (State*)(ws.p + o_exit0), a.exit[1] = (State*)(ws.p + o_exit1);
    a.last = (State*)(ws.p + o_last);
    a.count = (uint32_t*)(ws.p + o_count);
    a.first = (uint64_t*)(ws.p + o_first);
    a.flags = (uint32_t*)(ws.p + o_flags);
    a.coef = (int16_t*)(ws.p + o_coef);
    a.dcd = (uint32_t*)(ws.p + o_dcd);
    a.dcoff = (uint64_t*)(ws.p + o_dcoff);
    a.sums = (uint64_t*)(ws.p + o_sums);
    a.plane[0] = ws.p + o_p0;
    a.plane[1] = g.nc == 3 ? ws.p + o_p0 + p0_bytes : nullptr;
    a.plane[2] = g.nc == 3 ? ws.p + o_p0 + p0_bytes + pc_bytes : nullptr;
    a.out = (uint8_t*)out, a.pitch = pitch, a.out_cn = (uint32_t)out_cn;

    e = hipMemcpyAsync(ws.p, stage, up_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = hipMemsetAsync(a.flags, 0, 8, st);
    if (e == hipSuccess)
        e = hipMemsetAsync(a.flags + 2, 0xff, 4, st);  // kNoError
    if (e == hipSuccess)
        e = hipMemsetAsync(a.u, 0, u_bytes, st);
    if (e == hipSuccess)
        e = hipMemsetAsync(a.coef, 0, coef_bytes, st);
    if (e == hipSuccess)
        e = launch_unstuff(a, st);
    if (e == hipSuccess)
        e = launch_sync_init(a, st);
    // the rounds: at most nsub + 1, since round r fixes the first r entry states of every segment for good
    uint32_t r = 0;
    while (e == hipSuccess) {
        r++;
        e = launch_sync_round(a, r, st);
        if (e == hipSuccess)
            e = hipMemcpyAsync((void*)back, a.flags + (r & 1u), 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess)
            e = hipStreamSynchronize(st);
        if (e != hipSuccess || back[0] == 0 || r > nsub)
            break;
    }
    if (report)
        report->rounds = r;
    if (e == hipSuccess)
        e = launch_write(a, r, st);
    if (e == hipSuccess)
        e = hipMemcpyAsync((void*)back, a.flags + 2, 4, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);  // (also on an error above: nothing of this call is in flight when the lock goes)
    if (e == hipSuccess)
        e = es;
    if (e != hipSuccess)
        return set_error(V1C_E_HIP, std::string("v1c_jpeg_decode (kernels): ") + hipGetErrorString(e));
    if (back[0] != kNoError) {
        if (report)
            report->error_pos = back[0];
        return set_error(V1C_E_CORRUPT, "v1c_jpeg_decode: the entropy-coded data is damaged at bit " + std::to_string(back[0]) +
                                            " of the unstuffed scan");
    }
    e = launch_pixels(a, st);
    if (e != hipSuccess)
        return set_error(V1C_E_HIP, std::string("v1c_jpeg_decode (pixels): ") + hipGetErrorString(e));
    return V1C_OK;
}
