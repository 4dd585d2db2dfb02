// jpegdec.hip -- host side of the JPEG decoding entry points of the C ABI (v1c_jpeg_decode*, include/vr180_remap.h): the parse, the
// upload from the page-locked staging buffer, the chain of kernels and the rounds of the synchronisation, whose flag the host reads
// (jpegdec_launch.hpp: decode_to_coef, the step the lossless entries share); and the same for a batch of files in shared launches and rounds (v1c_jpeg_decode_batch); and for a progressive
// file scan by scan (v1c_jpeg_prog_decode).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/vr180_remap.h"
#include "host_util.hpp"
#include "jpegdec_host.hpp"
#include "jpegdec_launch.hpp"
#include "jpegprog_host.hpp"
#include "jpegprog_launch.hpp"

using namespace v1c;
using namespace v1c::jpegdec;

namespace {

// The page-locked staging buffers, one per device, grown on demand and kept: what is uploaded (tables, segment offsets, the scan) and
// the word that comes back.  Each has a lock of its own, held by a call from filling the buffer to its last synchronisation, so the
// buffer is never rewritten under a copy in flight: decodes on ONE device take turns (whatever their streams), decodes on different
// devices do not meet.
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

// the code of a parse that failed, and what it found
int parse_error(ParseResult r, const Parsed& p, std::string& why)
{
    why = p.why + " (byte " + std::to_string(p.error_pos) + ")";
    return r == kUnsupported ? V1C_E_UNSUPPORTED : V1C_E_CORRUPT;
}

// Whether a file can be decoded into its destination, for the single call and for every file of a batch: V1C_OK and the parse in ps, or
// the code and what is wrong.  Where the parse refused the file, ps.error_pos has the byte.
int file_error(const uint8_t* file, uint64_t size, const void* out, int64_t pitch, int out_cn, Parsed& ps, std::string& why)
{
    if (!file || !out)
        return why = "NULL pointer", V1C_E_INVALID;
    if (out_cn != 1 && out_cn != 3)
        return why = "out_cn must be 1 or 3", V1C_E_INVALID;
    const ParseResult pr = parse(file, size, ps);
    if (pr != kParsed)
        return parse_error(pr, ps, why);
    if (out_cn == 1 && ps.g.nc != 1)
        return why = "out_cn 1 takes a file of one component", V1C_E_INVALID;
    if (pitch < (int64_t)ps.g.w * out_cn)
        return why = "pitch is smaller than a row's bytes", V1C_E_INVALID;
    return V1C_OK;
}

}  // namespace

extern "C" int v1c_jpeg_decode_info(const uint8_t* file, uint64_t size, v1c_jpeg_info* info)
{
    if (!file || !info)
        return set_error(V1C_E_INVALID, "v1c_jpeg_decode_info: NULL pointer");
    Parsed p;
    const ParseResult r = parse(file, size, p);
    if (r != kParsed) {
        std::string why;
        const int code = parse_error(r, p, why);
        return set_error(code, "v1c_jpeg_decode_info: " + why);
    }
    info->height = (int32_t)p.g.h, info->width = (int32_t)p.g.w, info->components = (int32_t)p.g.nc;
    info->h_samp = (int32_t)p.g.hs, info->v_samp = (int32_t)p.g.vs, info->restart_interval = (int32_t)p.restart;
    return V1C_OK;
}

extern "C" int v1c_jpeg_decode(int device, void* stream, const uint8_t* file, uint64_t size, void* out, int64_t pitch, int out_cn,
                               uint32_t subseq_bits, v1c_jpeg_decode_report* report)
{
    if (report)
        std::memset(report, 0, sizeof(*report));
    const uint32_t S = subseq_of(subseq_bits);
    if (!S)
        return set_error(V1C_E_INVALID, std::string("v1c_jpeg_decode: ") + kSubseqRule);
    Parsed ps;
    std::string why;
    const int bad = file_error(file, size, out, pitch, out_cn, ps, why);
    if (bad != V1C_OK) {
        if (report)
            report->error_pos = ps.error_pos;
        return set_error(bad, "v1c_jpeg_decode: " + why);
    }
    const Geom& g = ps.g;

    if (device < 0 || device >= kMaxDevices)
        return set_error(V1C_E_NODEVICE, "v1c_jpeg_decode: no such device");
    DeviceGuard dg(device);
    if (!dg.ok)
        return set_error(V1C_E_NODEVICE, "hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    if (stream_is_capturing(st))
        return set_error(V1C_E_UNSUPPORTED, "v1c_jpeg_decode: the host reads a flag between the rounds, so the call cannot be captured into a graph");

    const std::vector<uint32_t> subfirst = sub_first(ps, S);
    const uint32_t nseg = g.nseg, nsub = subfirst.back();
    if (report)
        report->segments = nseg, report->subsequences = nsub;
    // the upload (tables, segment offsets, first subsequences, the scan) and behind it what the kernels make
    const Layout l = layout_of(ps, nsub);
    const size_t up_bytes = l.up_bytes;

    Staging& sg = g_staging[device];
    std::lock_guard<std::mutex> lock(sg.mu);
    uint8_t* stage = staging(sg, up_bytes + 64);
    if (!stage)
        return set_error(V1C_E_HIP, "v1c_jpeg_decode: hipHostMalloc of the staging buffer failed");
    std::memset(stage, 0, up_bytes);
    stage_file(stage, ps, l, subfirst, file);
    volatile uint32_t* back = (volatile uint32_t*)(stage + up_bytes);        // what comes back: a round's flag, the verdict

    Workspace ws(st);
    hipError_t e = hipMallocAsync((void**)&ws.p, l.bytes, st);
    if (e != hipSuccess)
        return set_error(V1C_E_HIP, std::string("v1c_jpeg_decode: hipMallocAsync: ") + hipGetErrorString(e));
    const Args a = args_of(ps, l, nsub, S, ws.p, ws.p + up_bytes, (uint32_t*)(ws.p + up_bytes + l.o_flags), out, pitch, out_cn);

    uint32_t r = 0;
    e = decode_to_coef(a, l, stage, nsub, st, back, &r);
    if (report)
        report->rounds = r;
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

namespace {

// one file of a batch that the parse accepted
struct BatchFile {
    int index;  // in the caller's arrays
    Parsed ps;
    std::vector<uint32_t> subfirst;
    uint32_t nsub = 0, rounds = 0;
    Layout l{};
    uint64_t groups[kWorkLists] = {};
};

uint64_t groups_of(uint64_t n, uint32_t per)
{
    return (n + per - 1) / per;
}

// One chunk: files [lo, hi) of `files` in one allocation, one upload and shared launches.  status / reports: the caller's arrays.
// Returns a HIP error, and the chunk's round launches in *rounds.
hipError_t decode_chunk(Staging& sg, hipStream_t st, std::vector<BatchFile>& files, size_t lo, size_t hi, const uint8_t* const* data,
                        void* const* outs, const int64_t* pitches, const int* out_cns, uint32_t S, int* status,
                        v1c_jpeg_decode_report* reports, uint32_t* rounds)
{
    const uint32_t n = (uint32_t)(hi - lo);
    // the chunk's head -- Args, work lists, last rounds, flags --, then every file's upload, then every file's work
    const size_t o_args = 0, o_first = o_args + align256((size_t)n * sizeof(Args)), o_rounds = o_first + align256((size_t)kWorkLists * (n + 1) * 4);
    const size_t o_flags = o_rounds + align256((size_t)n * 4), flag_bytes = (size_t)n * kFlagWords * 4;
    std::vector<size_t> o_up(n), o_work(n);
    size_t at = o_flags + align256(flag_bytes);
    for (uint32_t f = 0; f < n; f++)
        o_up[f] = at, at += files[lo + f].l.up_bytes;
    const size_t up_bytes = at;
    for (uint32_t f = 0; f < n; f++)
        o_work[f] = at, at += files[lo + f].l.work_bytes;
    const size_t bytes = at;

    uint8_t* stage = staging(sg, up_bytes + flag_bytes + 64);
    if (!stage)
        return hipErrorOutOfMemory;
    std::memset(stage, 0, up_bytes);
    Args* args = (Args*)(stage + o_args);
    uint32_t *first = (uint32_t*)(stage + o_first), *last_round = (uint32_t*)(stage + o_rounds), *flags = (uint32_t*)(stage + o_flags);
    volatile uint32_t* back = (volatile uint32_t*)(stage + up_bytes);  // what comes back: all the files' flags

    Workspace ws(st);
    hipError_t e = hipMallocAsync((void**)&ws.p, bytes, st);
    if (e != hipSuccess)
        return e;
    uint32_t most = 0;
    for (uint32_t f = 0; f < n; f++) {
        const BatchFile& bf = files[lo + f];
        args[f] = args_of(bf.ps, bf.l, bf.nsub, S, ws.p + o_up[f], ws.p + o_work[f], (uint32_t*)(ws.p + o_flags) + (size_t)f * kFlagWords,
                          outs[bf.index], pitches[bf.index], out_cns[bf.index]);
        stage_file(stage + o_up[f], bf.ps, bf.l, bf.subfirst, data[bf.index]);
        flags[f * kFlagWords + kErrSlot] = kNoError;
        for (int l = 0; l < kWorkLists; l++)
            first[(size_t)l * (n + 1) + f + 1] = first[(size_t)l * (n + 1) + f] + (uint32_t)bf.groups[l];
        most = std::max(most, bf.nsub);
    }
    std::vector<int> skip(n, 0);
    const Batch b{(const Args*)(ws.p + o_args), (const uint32_t*)(ws.p + o_first), (const uint32_t*)(ws.p + o_rounds), n};
    const BatchHost h{args, first, skip.data()};

    e = hipMemcpyAsync(ws.p, stage, up_bytes, hipMemcpyHostToDevice, st);
    for (uint32_t f = 0; f < n && e == hipSuccess; f++) {
        e = hipMemsetAsync(args[f].u, 0, files[lo + f].l.u_bytes, st);
        if (e == hipSuccess)
            e = hipMemsetAsync(args[f].coef, 0, files[lo + f].l.coef_bytes, st);
    }
    if (e == hipSuccess)
        e = launch_unstuff_batch(b, h, st);
    if (e == hipSuccess)
        e = launch_sync_init_batch(b, h, st);
    // the rounds: a file is done at its first quiet round or at its own bound, the chunk when all its files are
    uint32_t r = 0, open = n;
    while (e == hipSuccess && open) {
        r++;
        e = launch_sync_round_batch(b, h, r, st);
        if (e == hipSuccess)
            e = hipMemcpyAsync((void*)back, ws.p + o_flags, flag_bytes, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess)
            e = hipStreamSynchronize(st);
        if (e != hipSuccess)
            break;
        for (uint32_t f = 0; f < n; f++) {
            BatchFile& bf = files[lo + f];
            if (!bf.rounds && (back[f * kFlagWords + r % kRoundSlots] == 0 || r > bf.nsub))
                bf.rounds = r, open--;
        }
        if (r > most)
            break;
    }
    *rounds = r;
    for (uint32_t f = 0; f < n; f++)
        last_round[f] = reports[files[lo + f].index].rounds = files[lo + f].rounds;
    if (e == hipSuccess)
        e = hipMemcpyAsync(ws.p + o_rounds, last_round, (size_t)n * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = launch_write_batch(b, h, st);
    if (e == hipSuccess)
        e = hipMemcpyAsync((void*)back, ws.p + o_flags, flag_bytes, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);  // (also on an error above: nothing of this chunk reads the staging buffer after this)
    if (e == hipSuccess)
        e = es;
    if (e != hipSuccess)
        return e;
    for (uint32_t f = 0; f < n; f++) {
        const uint32_t err = back[f * kFlagWords + kErrSlot];
        if (err != kNoError) {
            skip[f] = 1;
            status[files[lo + f].index] = V1C_E_CORRUPT;
            reports[files[lo + f].index].error_pos = err;
        }
    }
    return launch_pixels_batch(b, h, st);
}

}  // namespace

extern "C" int v1c_jpeg_decode_batch(int device, void* stream, int n, const uint8_t* const* files, const uint64_t* sizes, void* const* outs,
                                     const int64_t* pitches, const int* out_cns, uint32_t subseq_bits, uint64_t max_workspace_bytes,
                                     int* status, v1c_jpeg_decode_report* reports, uint32_t* batch_rounds)
{
    if (batch_rounds)
        *batch_rounds = 0;
    if (n < 0)
        return set_error(V1C_E_INVALID, "v1c_jpeg_decode_batch: n is negative");
    if (n == 0)
        return V1C_OK;
    if (!files || !sizes || !outs || !pitches || !out_cns || !status || !reports)
        return set_error(V1C_E_INVALID, "v1c_jpeg_decode_batch: NULL pointer");
    const uint32_t S = subseq_of(subseq_bits);
    if (!S)
        return set_error(V1C_E_INVALID, std::string("v1c_jpeg_decode_batch: ") + kSubseqRule);
    // (device and capture first: under capture nothing is done, not even a status written)
    if (device < 0 || device >= kMaxDevices)
        return set_error(V1C_E_NODEVICE, "v1c_jpeg_decode_batch: no such device");
    DeviceGuard dg(device);
    if (!dg.ok)
        return set_error(V1C_E_NODEVICE, "hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    if (stream_is_capturing(st))
        return set_error(V1C_E_UNSUPPORTED, "v1c_jpeg_decode_batch: the host reads a flag between the rounds, so the call cannot be captured into a graph");
    std::memset(reports, 0, sizeof(*reports) * (size_t)n);

    // every file's arguments and parse, before the device is touched: a file refused here has its status and is left out
    std::vector<BatchFile> good;
    good.reserve((size_t)n);
    for (int i = 0; i < n; i++) {
        good.emplace_back();
        BatchFile& bf = good.back();
        std::string why;  // (a file of a batch has a status, no message)
        status[i] = file_error(files[i], sizes[i], outs[i], pitches[i], out_cns[i], bf.ps, why);
        if (status[i] != V1C_OK) {
            reports[i].error_pos = bf.ps.error_pos;
            good.pop_back();
            continue;
        }
        const Geom& g = bf.ps.g;
        bf.index = i;
        bf.subfirst = sub_first(bf.ps, S);
        bf.nsub = bf.subfirst.back();
        bf.l = layout_of(bf.ps, bf.nsub);
        bf.groups[kByPiece] = groups_of(bf.l.pieces, 256), bf.groups[kBySub] = groups_of(bf.nsub, 256);
        bf.groups[kByBlock] = groups_of(g.nblocks, 256), bf.groups[kByTile] = groups_of(g.nblocks, 32);
        bf.groups[kByPixel] = groups_of((uint64_t)((g.w + 3) / 4) * g.h, 256);
        reports[i].segments = g.nseg, reports[i].subsequences = bf.nsub;
    }
    if (good.empty())
        return V1C_OK;

    std::vector<uint64_t> bytes, groups;
    for (const BatchFile& bf : good) {
        bytes.push_back(bf.l.bytes + sizeof(Args) + 1024);  // (with the file's share of the chunk's head)
        groups.push_back(*std::max_element(bf.groups, bf.groups + kWorkLists));
    }
    Staging& sg = g_staging[device];
    std::lock_guard<std::mutex> lock(sg.mu);
    size_t lo = 0;
    uint32_t chunk = 0;
    for (uint32_t hi : chunk_ends(bytes, groups, max_workspace_bytes ? max_workspace_bytes : kDefaultBatchWorkspace)) {
        for (size_t f = lo; f < hi; f++)
            reports[good[f].index].reserved = chunk;
        uint32_t rounds = 0;
        const hipError_t e = decode_chunk(sg, st, good, lo, hi, files, outs, pitches, out_cns, S, status, reports, &rounds);
        if (batch_rounds)
            *batch_rounds += rounds;
        if (e != hipSuccess)
            return set_error(V1C_E_HIP, std::string("v1c_jpeg_decode_batch (chunk ") + std::to_string(chunk) + "): " + hipGetErrorString(e));
        lo = hi, chunk++;
    }
    return V1C_OK;
}

// ---- progressive files: the scans one after another into one coefficient store, then the sequential pixel stage -----------------------

extern "C" int v1c_jpeg_prog_info(const uint8_t* file, uint64_t size, v1c_jpeg_prog_info_t* info)
{
    if (!file || !info)
        return set_error(V1C_E_INVALID, "v1c_jpeg_prog_info: NULL pointer");
    std::memset(info, 0, sizeof(*info));
    jpegprog::PParsed p;
    const ParseResult r = jpegprog::parse(file, size, p);
    if (r != kParsed) {
        info->error_pos = p.error_pos;
        return set_error(r == kUnsupported ? V1C_E_UNSUPPORTED : V1C_E_CORRUPT,
                         "v1c_jpeg_prog_info: " + p.why + " (byte " + std::to_string(p.error_pos) + ")");
    }
    info->height = (int32_t)p.g.h, info->width = (int32_t)p.g.w, info->components = (int32_t)p.g.nc;
    info->h_samp = (int32_t)p.g.hs, info->v_samp = (int32_t)p.g.vs, info->scans = (int32_t)p.scans.size();
    return V1C_OK;
}

extern "C" int v1c_jpeg_prog_decode(int device, void* stream, const uint8_t* file, uint64_t size, void* out, int64_t pitch, int out_cn,
                                    uint32_t subseq_bits, v1c_jpeg_prog_report* report, uint32_t* scan_rounds, uint32_t scan_cap)
{
    namespace jp = jpegprog;
    if (report)
        std::memset(report, 0, sizeof(*report));
    const uint32_t S = subseq_of(subseq_bits);
    if (!S)
        return set_error(V1C_E_INVALID, std::string("v1c_jpeg_prog_decode: ") + kSubseqRule);
    if (!file || !out)
        return set_error(V1C_E_INVALID, "v1c_jpeg_prog_decode: NULL pointer");
    if (out_cn != 1 && out_cn != 3)
        return set_error(V1C_E_INVALID, "v1c_jpeg_prog_decode: out_cn must be 1 or 3");
    if (scan_cap && !scan_rounds)
        return set_error(V1C_E_INVALID, "v1c_jpeg_prog_decode: scan_cap without scan_rounds");
    jp::PParsed ps;
    const ParseResult pr = jp::parse(file, size, ps);
    if (pr != kParsed) {
        if (report)
            report->error_pos = ps.error_pos;
        return set_error(pr == kUnsupported ? V1C_E_UNSUPPORTED : V1C_E_CORRUPT,
                         "v1c_jpeg_prog_decode: " + ps.why + " (byte " + std::to_string(ps.error_pos) + ")");
    }
    const Geom& g = ps.g;
    if (out_cn == 1 && g.nc != 1)
        return set_error(V1C_E_INVALID, "v1c_jpeg_prog_decode: out_cn 1 takes a file of one component");
    if (pitch < (int64_t)g.w * out_cn)
        return set_error(V1C_E_INVALID, "v1c_jpeg_prog_decode: pitch is smaller than a row's bytes");

    if (device < 0 || device >= kMaxDevices)
        return set_error(V1C_E_NODEVICE, "v1c_jpeg_prog_decode: no such device");
    DeviceGuard dg(device);
    if (!dg.ok)
        return set_error(V1C_E_NODEVICE, "hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    if (stream_is_capturing(st))
        return set_error(V1C_E_UNSUPPORTED, "v1c_jpeg_prog_decode: the host reads a flag between the rounds, so the call cannot be captured into a graph");

    // the upload: the pixel stage's quantisation tables, then every scan's tables, segment offsets, first subsequences and bytes; behind it
    // the work, every buffer as large as the scan that needs it most
    const size_t nscan = ps.scans.size();
    struct Up {
        size_t o_tab, o_segoff, o_subfirst, o_scan;
        uint32_t pieces, nsub;
        std::vector<uint32_t> subfirst;
    };
    std::vector<Up> up(nscan);
    size_t at = align256(sizeof(Tables));
    uint64_t pieces = 0, nu = 0, nsub = 0, nsub_all = 0, nseg_all = 0;
    for (size_t s = 0; s < nscan; s++) {
        const jp::PScan& sc = ps.scans[s];
        Up& x = up[s];
        x.subfirst = jp::sub_first(sc, S);
        x.nsub = x.subfirst.back(), x.pieces = ((uint32_t)sc.scan_len + kPiece - 1) / kPiece;
        const size_t nseg = sc.sc.nseg;
        x.o_tab = at, x.o_segoff = x.o_tab + align256(sizeof(Tables)), x.o_subfirst = x.o_segoff + align256((nseg + 1) * 4);
        x.o_scan = x.o_subfirst + align256((nseg + 1) * 4), at = x.o_scan + align256(((size_t)x.pieces + 1) * kPiece);
        pieces = std::max<uint64_t>(pieces, x.pieces), nu = std::max<uint64_t>(nu, sc.segoff.back()), nsub = std::max<uint64_t>(nsub, x.nsub);
        nsub_all += x.nsub, nseg_all += nseg;
    }
    const size_t up_bytes = at;
    if (report)
        report->scans = (uint32_t)nscan, report->segments = (uint32_t)nseg_all, report->subsequences = (uint32_t)nsub_all;
    const uint64_t nmax = std::max(std::max(pieces, nsub), (uint64_t)g.nblocks);
    const size_t o_flags = 0, o_drop = 256, o_dropoff = o_drop + align256(pieces * 4), o_u = o_dropoff + align256((pieces + 1) * 8);
    const size_t u_all = align256(nu + 16), o_exit0 = o_u + u_all, st_bytes = align256(nsub * sizeof(jp::PState));
    const size_t o_exit1 = o_exit0 + st_bytes, o_last = o_exit1 + st_bytes, o_count = o_last + st_bytes;
    const size_t o_first = o_count + align256(nsub * 4), o_coef = o_first + align256((nsub + 1) * 8);
    const size_t coef_bytes = align256((size_t)g.nblocks * 128), o_dd = o_coef + coef_bytes, o_ddoff = o_dd + align256((size_t)g.nblocks * 4);
    const size_t o_dcd = o_ddoff + align256(((size_t)g.nblocks + 1) * 8), o_dcoff = o_dcd + align256((size_t)g.nblocks * 4);
    const size_t o_sums = o_dcoff + align256(((size_t)g.nblocks + 1) * 8), o_p0 = o_sums + align256((nmax / jpeg::kScanChunk + 2) * 8);
    const size_t p0_bytes = align256((size_t)plane_pitch(g, 0) * plane_rows(g, 0)), pc_bytes = align256((size_t)plane_pitch(g, 1) * plane_rows(g, 1));
    const size_t work_bytes = o_p0 + p0_bytes + (g.nc == 3 ? 2 * pc_bytes : 0);

    Staging& sg = g_staging[device];
    std::lock_guard<std::mutex> lock(sg.mu);
    uint8_t* stage = staging(sg, up_bytes + 64);
    if (!stage)
        return set_error(V1C_E_HIP, "v1c_jpeg_prog_decode: hipHostMalloc of the staging buffer failed");
    std::memset(stage, 0, up_bytes);
    std::memcpy(stage, &ps.tab, sizeof(Tables));
    for (size_t s = 0; s < nscan; s++) {
        const jp::PScan& sc = ps.scans[s];
        const size_t nseg = sc.sc.nseg;
        std::memcpy(stage + up[s].o_tab, &sc.tab, sizeof(Tables));
        std::memcpy(stage + up[s].o_segoff, sc.segoff.data(), (nseg + 1) * 4);
        std::memcpy(stage + up[s].o_subfirst, up[s].subfirst.data(), (nseg + 1) * 4);
        std::memcpy(stage + up[s].o_scan, file + sc.scan_start, (size_t)sc.scan_len + 2);  // (the parse saw the marker behind the scan)
    }
    volatile uint32_t* back = (volatile uint32_t*)(stage + up_bytes);  // what comes back: a round's flag, a scan's verdict

    Workspace ws(st);
    hipError_t e = hipMallocAsync((void**)&ws.p, up_bytes + work_bytes, st);
    if (e != hipSuccess)
        return set_error(V1C_E_HIP, std::string("v1c_jpeg_prog_decode: hipMallocAsync: ") + hipGetErrorString(e));
    uint8_t* work = ws.p + up_bytes;
    Args ja{};  // the sequential decoder's: for its unstuffing kernels and its pixel stage
    ja.g = g, ja.tab = (const Tables*)ws.p;
    ja.drop = (uint32_t*)(work + o_drop), ja.dropoff = (uint64_t*)(work + o_dropoff), ja.u = (uint32_t*)(work + o_u);
    ja.flags = (uint32_t*)(work + o_flags), ja.coef = (int16_t*)(work + o_coef);
    ja.dcd = (uint32_t*)(work + o_dcd), ja.dcoff = (uint64_t*)(work + o_dcoff), ja.sums = (uint64_t*)(work + o_sums);
    ja.plane[0] = work + o_p0;
    ja.plane[1] = g.nc == 3 ? work + o_p0 + p0_bytes : nullptr;
    ja.plane[2] = g.nc == 3 ? work + o_p0 + p0_bytes + pc_bytes : nullptr;
    ja.out = (uint8_t*)out, ja.pitch = pitch, ja.out_cn = (uint32_t)out_cn;
    jp::ScanArgs a{};
    a.g = g, a.u = ja.u, a.S = S;
    a.exit[0] = (jp::PState*)(work + o_exit0), a.exit[1] = (jp::PState*)(work + o_exit1), a.last = (jp::PState*)(work + o_last);
    a.count = (uint32_t*)(work + o_count), a.first = (uint64_t*)(work + o_first), a.flags = ja.flags, a.coef = ja.coef;
    a.dd = (uint32_t*)(work + o_dd), a.ddoff = (uint64_t*)(work + o_ddoff), a.sums = ja.sums;

    e = hipMemcpyAsync(ws.p, stage, up_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = hipMemsetAsync(a.coef, 0, coef_bytes, st);
    uint32_t rounds_all = 0, bad_scan = 0, bad_bit = kNoError;
    for (size_t s = 0; s < nscan && e == hipSuccess && bad_bit == kNoError; s++) {
        const jp::PScan& sc = ps.scans[s];
        ja.scan = ws.p + up[s].o_scan, ja.scan_len = (uint32_t)sc.scan_len, ja.pieces = up[s].pieces;
        a.sc = sc.sc, a.tab = (const Tables*)(ws.p + up[s].o_tab);
        a.segoff = (const uint32_t*)(ws.p + up[s].o_segoff), a.subfirst = (const uint32_t*)(ws.p + up[s].o_subfirst), a.nsub = up[s].nsub;
        e = hipMemsetAsync(a.flags, 0, 8, st);
        if (e == hipSuccess)
            e = hipMemsetAsync(a.flags + 2, 0xff, 4, st);  // kNoError
        if (e == hipSuccess)
            e = hipMemsetAsync(ja.u, 0, align256((size_t)sc.segoff.back() + 16), st);
        if (e == hipSuccess)
            e = launch_unstuff(ja, st);
        if (e == hipSuccess)
            e = jp::launch_init(a, st);
        // the rounds: at most nsub + 1, since round r fixes the first r entry states of every segment for good
        uint32_t r = 0;
        while (e == hipSuccess) {
            r++;
            e = jp::launch_round(a, r, st);
            if (e == hipSuccess)
                e = hipMemcpyAsync((void*)back, a.flags + (r & 1u), 4, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess)
                e = hipStreamSynchronize(st);
            if (e != hipSuccess || back[0] == 0 || r > a.nsub)
                break;
        }
        rounds_all += r;
        if (s < scan_cap)
            scan_rounds[s] = r;
        if (e == hipSuccess)
            e = jp::launch_write(a, r, st);
        if (e == hipSuccess)
            e = hipMemcpyAsync((void*)back, a.flags + 2, 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess)
            e = hipStreamSynchronize(st);
        if (e == hipSuccess && back[0] != kNoError)
            bad_scan = (uint32_t)s, bad_bit = back[0];
    }
    if (e == hipSuccess && bad_bit == kNoError)
        e = jp::launch_dcdiff(a, st);
    const hipError_t es = hipStreamSynchronize(st);  // (also on an error above: nothing of this call is in flight when the lock goes)
    if (e == hipSuccess)
        e = es;
    if (report)
        report->rounds = rounds_all;
    if (e != hipSuccess)
        return set_error(V1C_E_HIP, std::string("v1c_jpeg_prog_decode (kernels): ") + hipGetErrorString(e));
    if (bad_bit != kNoError) {
        if (report)
            report->error_pos = bad_bit, report->error_scan = bad_scan;
        return set_error(V1C_E_CORRUPT, "v1c_jpeg_prog_decode: the entropy-coded data is damaged at bit " + std::to_string(bad_bit) +
                                            " of unstuffed scan " + std::to_string(bad_scan));
    }
    e = launch_pixels(ja, st);
    if (e != hipSuccess)
        return set_error(V1C_E_HIP, std::string("v1c_jpeg_prog_decode (pixels): ") + hipGetErrorString(e));
    return V1C_OK;
}
