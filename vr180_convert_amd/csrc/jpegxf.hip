// jpegxf.hip -- host side of the lossless JPEG composer's entry points of the C ABI (v1c_jpeg_compose*, v1c_jpeg_header_xf,
// include/vr180_remap.h): the parse of every source and the rules of the outputs, all before the device is touched; then every
// source's decode in turn up to its DC scan -- the decoder's chain with the rounds the host reads a flag between, each into a
// coefficient store of its own --, the gather of every output from those stores, one synchronisation for every verdict, and the
// batch encoder's chain from a filled coefficient store on (jpegxc_launch.hpp: launch_encode_coef), as it is.  INTEGRATION.md
// section 10 has the contract, DESIGN.md section 20 the design.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/vr180_remap.h"
#include "host_util.hpp"
#include "jpeg_host.hpp"
#include "jpegxc_launch.hpp"
#include "jpegxf_host.hpp"
#include "jpegxf_launch.hpp"

using namespace v1c;
using namespace v1c::jpegxf;

namespace {

constexpr int kMaxDevices = 64;

// what the host-only checks of a call give: the parses, and every output's geometry and regions
struct Checked {
    std::vector<jpegdec::Parsed> ps;
    std::vector<jpeg::Geom> geoms;
    std::vector<RegionList> lists;
};

// the parse and the file's scope: V1C_OK, or the code and why
int file_error(const uint8_t* file, uint64_t size, jpegdec::Parsed& ps, std::string& why)
{
    if (!file)
        return why = "NULL pointer", V1C_E_INVALID;
    const jpegdec::ParseResult pr = jpegdec::parse(file, size, ps);
    if (pr != jpegdec::kParsed) {
        why = ps.why + " (byte " + std::to_string(ps.error_pos) + ")";
        return pr == jpegdec::kUnsupported ? V1C_E_UNSUPPORTED : V1C_E_CORRUPT;
    }
    return jpegxc::source_error(ps, why);
}

// every check that needs no device; buffers: whether out_host and capacity count
int call_error(int nsources, const v1c_jpeg_xf_source* sources, int n, const v1c_jpeg_xf_output* outputs, bool buffers, Checked& c, std::string& why)
{
    if (!sources || nsources < 1 || nsources > V1C_JPEG_XF_MAX_SOURCES)
        return why = "1 ... " + std::to_string(V1C_JPEG_XF_MAX_SOURCES) + " sources", V1C_E_INVALID;
    if (!outputs || n < 1 || n > V1C_JPEG_XC_MAX_OUTPUTS)
        return why = "1 ... " + std::to_string(V1C_JPEG_XC_MAX_OUTPUTS) + " outputs", V1C_E_INVALID;
    c.ps.resize((size_t)nsources);
    for (int i = 0; i < nsources; i++) {
        const int bad = file_error(sources[i].file, sources[i].size, c.ps[(size_t)i], why);
        if (bad != V1C_OK)
            return why = "source " + std::to_string(i) + ": " + why, bad;
    }
    const int bad = sources_error(c.ps, why);
    if (bad != V1C_OK)
        return bad;
    c.geoms.resize((size_t)n), c.lists.resize((size_t)n);
    for (int i = 0; i < n; i++) {
        std::string w;
        const int rc = check_output(c.ps, outputs[i], c.geoms[(size_t)i], c.lists[(size_t)i], w);
        if (rc != V1C_OK)
            return why = "output " + std::to_string(i) + ": " + w, rc;
        if (buffers && (!outputs[i].out_host || outputs[i].capacity < jpeg::scan_bound(c.geoms[(size_t)i])))
            return why = "output " + std::to_string(i) + ": NULL out_host, or capacity below v1c_jpeg_compose_bound = " +
                         std::to_string(jpeg::scan_bound(c.geoms[(size_t)i])),
                   V1C_E_INVALID;
    }
    return V1C_OK;
}

// The tables an output's stages read: the Annex K codes (an optimising output's are overwritten on the device); the quantiser half,
// which no stage behind the transform reads, is that of the output's header
void make_tables(const jpegdec::Parsed& ps, bool transposed, jpeg::Tables& t)
{
    effective_tables(ps, transposed, t.q);
    jpeg::code_table(jpeg::kDcLuma, t.dc[0], 16);
    jpeg::code_table(jpeg::kDcChroma, t.dc[1], 16);
    jpeg::code_table(jpeg::kAcLuma, t.ac[0], 256);
    jpeg::code_table(jpeg::kAcChroma, t.ac[1], 256);
}

// one source's part of the workspace and of the call
struct Decode {
    std::vector<uint32_t> subfirst;
    uint32_t nsub = 0;
    jpegdec::Layout l;
    size_t at = 0, bytes = 0;       // in the workspace
    std::vector<uint8_t> stage;     // (pageable: alive until the call's last synchronisation)
    jpegdec::Args a;
};

}  // namespace

extern "C" uint64_t v1c_jpeg_compose_bound(const uint8_t* file, uint64_t size, int width, int height, int restart_mcus)
{
    jpegdec::Parsed ps;
    std::string why;
    jpeg::Geom g;
    if (file_error(file, size, ps, why) != V1C_OK || !jpegxc::out_geom(ps.g, width, height, restart_mcus, g))
        return 0;
    return jpeg::scan_bound(g);
}

extern "C" int v1c_jpeg_compose_check(int nsources, const v1c_jpeg_xf_source* sources, int n, const v1c_jpeg_xf_output* outputs, uint64_t* error_pos)
{
    Checked c;
    std::string why;
    const int bad = call_error(nsources, sources, n, outputs, false, c, why);
    if (error_pos && nsources >= 1 && nsources <= V1C_JPEG_XF_MAX_SOURCES)
        for (int i = 0; i < nsources; i++)
            error_pos[i] = (size_t)i < c.ps.size() ? c.ps[(size_t)i].error_pos : 0;
    return bad == V1C_OK ? V1C_OK : set_error(bad, "v1c_jpeg_compose_check: " + why);
}

extern "C" int64_t v1c_jpeg_header_xf(const uint8_t* file, uint64_t size, int width, int height, int restart_mcus, int transposed,
                                      const uint8_t* dht, uint32_t dht_size, uint8_t* out, uint64_t capacity)
{
    jpegdec::Parsed ps;
    std::string why;
    const int bad = file_error(file, size, ps, why);
    if (bad != V1C_OK)
        return set_error(bad, "v1c_jpeg_header_xf: " + why);
    jpeg::Geom g;
    if (!out || !jpegxc::out_geom(ps.g, width, height, restart_mcus, g))
        return set_error(V1C_E_INVALID, "v1c_jpeg_header_xf: NULL pointer, or sizes or restart_mcus out of range");
    if (transposed && ps.g.hs != ps.g.vs)
        return set_error(V1C_E_UNSUPPORTED, "v1c_jpeg_header_xf: a transposed 4:2:2 file would be 4:4:0, which neither codec handles");
    if (dht && (dht_size > V1C_JPEG_DHT_MAX || !jpegxc::whole_tables(dht, dht_size, ps.g.nc)))
        return set_error(V1C_E_INVALID, "v1c_jpeg_header_xf: dht is not the tables of an optimising output of such a file");
    const std::vector<uint8_t> head = xf_header(ps, transposed != 0, g, restart_mcus, dht, dht_size);
    if (capacity < head.size())
        return set_error(V1C_E_INVALID, "v1c_jpeg_header_xf: capacity is below V1C_JPEG_HEADER_XC_MAX");
    std::memcpy(out, head.data(), head.size());
    return (int64_t)head.size();
}

extern "C" int v1c_jpeg_compose(int device, void* stream, int nsources, const v1c_jpeg_xf_source* sources, int n, v1c_jpeg_xf_output* outputs,
                                uint32_t subseq_bits, v1c_jpeg_decode_report* reports)
{
    using jpeg::Image;
    using jpeg::Tables;
    const bool counted = nsources >= 1 && nsources <= V1C_JPEG_XF_MAX_SOURCES;
    if (reports && counted)
        std::memset(reports, 0, sizeof(*reports) * (size_t)nsources);
    const uint32_t S = subseq_bits ? subseq_bits : jpegdec::kDefaultSubseqBits;
    if (S % 32 || S < 256 || S > (1u << 24))
        return set_error(V1C_E_INVALID, "v1c_jpeg_compose: subseq_bits must be a multiple of 32 from 256 to 2^24, or 0");
    Checked c;
    std::string why;
    const int bad = call_error(nsources, sources, n, outputs, true, c, why);
    if (bad != V1C_OK) {
        if (reports && counted)
            for (size_t i = 0; i < c.ps.size(); i++)
                reports[i].error_pos = c.ps[i].error_pos;
        return set_error(bad, "v1c_jpeg_compose: " + why);
    }
    const jpegdec::Geom& sg = c.ps[0].g;  // (components, sampling factors and blocks per MCU: those of every source)

    if (device < 0 || device >= kMaxDevices)
        return set_error(V1C_E_NODEVICE, "v1c_jpeg_compose: no such device");
    DeviceGuard dg(device);
    if (!dg.ok)
        return set_error(V1C_E_NODEVICE, "hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    if (stream_is_capturing(st))
        return set_error(V1C_E_UNSUPPORTED, "v1c_jpeg_compose: the host reads a flag between the rounds and the sizes between the kernels and the "
                                            "copies, so the call cannot be captured into a graph");
    for (int i = 0; i < n; i++)
        outputs[i].size = 0, outputs[i].dht_size = 0;

    // the decoders' parts of the workspace, one per source: its upload, and its work up to the planes, which no pixel stage fills here
    const uint32_t us = (uint32_t)nsources;
    std::vector<Decode> dec(us);
    size_t dec_bytes = 0;
    for (uint32_t i = 0; i < us; i++) {
        Decode& d = dec[i];
        d.subfirst = jpegdec::sub_first(c.ps[i], S);
        d.nsub = d.subfirst.back();
        if (reports)
            reports[i].segments = c.ps[i].g.nseg, reports[i].subsequences = d.nsub;
        d.l = jpegdec::layout_of(c.ps[i], d.nsub);
        d.at = dec_bytes, d.bytes = align256(d.l.up_bytes + d.l.o_p0);
        dec_bytes += d.bytes;
    }

    // the encoder's part, laid out as v1c_jpeg_transcode lays it out
    const uint32_t un = (uint32_t)n;
    std::vector<int32_t> slot_of(un, -1);
    std::vector<jpeg::OptSlot> slots;
    for (uint32_t f = 0; f < un; f++)
        if (outputs[f].optimize) {
            slot_of[f] = (int32_t)slots.size();
            slots.push_back(jpeg::OptSlot{f, sg.nc == 1 ? 2u : 4u});
        }
    const size_t nslots = slots.size();
    const size_t o_im = 0, o_first = o_im + align256((size_t)un * sizeof(Image)), o_tabs = o_first + align256((size_t)jpeg::kWorkLists * (un + 1) * 4);
    const size_t o_slotof = o_tabs + align256((size_t)un * sizeof(Tables)), o_slots = o_slotof + align256((size_t)un * 4);
    const size_t o_sizes = o_slots + align256((nslots + 1) * sizeof(jpeg::OptSlot));
    const size_t o_rec = o_sizes + align256((size_t)un * 8), o_hist = o_rec + align256(nslots * sizeof(jpeg::DhtRecord));
    const size_t o_flag = o_hist + align256(nslots * sizeof(jpeg::Hist)), head = o_flag + 256;
    const size_t back_bytes = nslots ? o_rec + nslots * sizeof(jpeg::DhtRecord) - o_sizes : (size_t)un * 8;
    std::vector<uint8_t> up(o_sizes, 0);  // (pageable, as the decoders' uploads: alive until the call's last synchronisation)
    Image* im = (Image*)(up.data() + o_im);
    uint32_t* first = (uint32_t*)(up.data() + o_first);
    for (uint32_t f = 0; f < un; f++) {
        const Region& r0 = c.lists[f].r[0];
        im[f].img = nullptr, im[f].pitch = 0, im[f].g = c.geoms[f], im[f].tab = f;
        make_tables(c.ps[r0.source], (r0.code & kTranspose) != 0, ((Tables*)(up.data() + o_tabs))[f]);
    }
    const jpeg::Totals t = jpeg::place_regions(im, un, first);
    std::memcpy(up.data() + o_slotof, slot_of.data(), (size_t)un * 4);
    if (nslots)
        std::memcpy(up.data() + o_slots, slots.data(), nslots * sizeof(jpeg::OptSlot));
    const size_t raw_bytes = align256(t.pieces * jpeg::kPiece + 16);
    const size_t o_coef = head, o_bits = o_coef + align256(t.nblocks * 128), o_bitoff = o_bits + align256(t.nblocks * 4);
    const size_t o_ibytes = o_bitoff + align256((t.nblocks + 1) * 8), o_ioff = o_ibytes + align256(t.nint * 4);
    const size_t o_raw = o_ioff + align256((t.nint + 1) * 8), o_ffcnt = o_raw + raw_bytes, o_ffoff = o_ffcnt + align256(t.pieces * 4);
    const size_t o_sums = o_ffoff + align256((t.pieces + 1) * 8), o_out = o_sums + align256(jpeg::sums_of(t, jpeg::kScanChunk) * 8);
    const size_t enc_bytes = o_out + align256(t.out_bytes + 8);

    for (uint32_t i = 0; i < us; i++) {
        dec[i].stage.assign(dec[i].l.up_bytes, 0);
        jpegdec::stage_file(dec[i].stage.data(), c.ps[i], dec[i].l, dec[i].subfirst, sources[i].file);
    }

    Workspace ws(st);
    hipError_t e = hipMallocAsync((void**)&ws.p, dec_bytes + enc_bytes, st);
    if (e != hipSuccess)
        return set_error(V1C_E_HIP, std::string("v1c_jpeg_compose: hipMallocAsync: ") + hipGetErrorString(e));
    uint8_t* enc = ws.p + dec_bytes;
    jpeg::Batch b{};
    b.im = (const Image*)(enc + o_im), b.first = (const uint32_t*)(enc + o_first), b.tabs = (const Tables*)(enc + o_tabs);
    b.n = un, b.t = t;
    b.sizes = (uint64_t*)(enc + o_sizes);
    b.buf.coef = (int16_t*)(enc + o_coef), b.buf.bits = (uint32_t*)(enc + o_bits), b.buf.bitoff = (uint64_t*)(enc + o_bitoff);
    b.buf.ibytes = (uint32_t*)(enc + o_ibytes), b.buf.ioff = (uint64_t*)(enc + o_ioff), b.buf.raw = (uint32_t*)(enc + o_raw);
    b.buf.ffcnt = (uint32_t*)(enc + o_ffcnt), b.buf.ffoff = (uint64_t*)(enc + o_ffoff), b.buf.sums = (uint64_t*)(enc + o_sums);
    b.buf.out = enc + o_out;
    jpeg::OptBatch o{};
    o.slot_of = (const int32_t*)(enc + o_slotof), o.slots = (const jpeg::OptSlot*)(enc + o_slots), o.nslots = (uint32_t)nslots;
    o.hist = (jpeg::Hist*)(enc + o_hist), o.rec = (jpeg::DhtRecord*)(enc + o_rec), o.tabs = (Tables*)(enc + o_tabs);
    uint32_t* xflag = (uint32_t*)(enc + o_flag);

    e = hipMemcpyAsync(enc, up.data(), o_sizes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = hipMemsetAsync(b.buf.raw, 0, raw_bytes, st);
    if (e == hipSuccess)
        e = hipMemsetAsync(b.sizes, 0, head - o_sizes, st);

    // every source's decode up to the coefficients and its DC scan, in turn; what comes back meanwhile: a round's flag
    uint32_t back[V1C_JPEG_XF_MAX_SOURCES + 1] = {0, 0, 0, 0, 0};
    for (uint32_t i = 0; i < us && e == hipSuccess; i++) {
        Decode& d = dec[i];
        uint8_t* base = ws.p + d.at;
        d.a = jpegdec::args_of(c.ps[i], d.l, d.nsub, S, base, base + d.l.up_bytes, (uint32_t*)(base + d.l.up_bytes + d.l.o_flags), nullptr, 0, 3);
        const jpegdec::Args& a = d.a;
        e = hipMemcpyAsync(base, d.stage.data(), d.l.up_bytes, hipMemcpyHostToDevice, st);
        if (e == hipSuccess)
            e = hipMemsetAsync(a.flags, 0, 8, st);
        if (e == hipSuccess)
            e = hipMemsetAsync(a.flags + 2, 0xff, 4, st);  // kNoError
        if (e == hipSuccess)
            e = hipMemsetAsync(a.u, 0, d.l.u_bytes, st);
        if (e == hipSuccess)
            e = hipMemsetAsync(a.coef, 0, d.l.coef_bytes, st);
        if (e == hipSuccess)
            e = jpegdec::launch_unstuff(a, st);
        if (e == hipSuccess)
            e = jpegdec::launch_sync_init(a, st);
        // the rounds: at most nsub + 1, since round r fixes the first r entry states of every segment for good
        uint32_t r = 0, more = 0;
        while (e == hipSuccess) {
            r++;
            e = jpegdec::launch_sync_round(a, r, st);
            if (e == hipSuccess)
                e = hipMemcpyAsync(&more, a.flags + (r & 1u), 4, hipMemcpyDeviceToHost, st);
            if (e == hipSuccess)
                e = hipStreamSynchronize(st);
            if (e != hipSuccess || more == 0 || r > d.nsub)
                break;
        }
        if (reports)
            reports[i].rounds = r;
        if (e == hipSuccess)
            e = jpegdec::launch_write(a, r, st);
        // (as in v1c_jpeg_transcode the DC scan and the gathers are queued before the decoder's error word is read: on a damaged scan
        //  they run over whatever the last pass left, which is safe -- every index comes from the geometry, never from the data, and
        //  every load stays inside the source's zeroed store)
        if (e == hipSuccess)
            e = jpegxc::launch_dc(a, st);
    }
    for (uint32_t f = 0; f < un && e == hipSuccess; f++) {
        GatherArgs ga{};
        for (uint32_t i = 0; i < us; i++)
            ga.src[i].coef = dec[i].a.coef, ga.src[i].dcoff = dec[i].a.dcoff, ga.src[i].g = c.ps[i].g;
        ga.dst = b.buf.coef + (size_t)im[f].blk0 * 64, ga.dst_mcux = im[f].g.mcux, ga.dst_nblocks = im[f].g.nblocks;
        ga.flag = xflag, ga.regions = c.lists[f];
        e = launch_gather(ga, st);
    }
    // one synchronisation for every verdict: each source's error word, and the gathers' range flag
    for (uint32_t i = 0; i < us && e == hipSuccess; i++)
        e = hipMemcpyAsync(&back[i], dec[i].a.flags + 2, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess)
        e = hipMemcpyAsync(&back[V1C_JPEG_XF_MAX_SOURCES], xflag, 4, hipMemcpyDeviceToHost, st);
    const hipError_t ev = hipStreamSynchronize(st);  // (also on an error above: nothing of this call reads the host's buffers after it)
    if (e == hipSuccess)
        e = ev;
    if (e != hipSuccess)
        return set_error(V1C_E_HIP, std::string("v1c_jpeg_compose (decode): ") + hipGetErrorString(e));
    int damaged = -1;
    for (uint32_t i = 0; i < us; i++)
        if (back[i] != jpegdec::kNoError) {
            if (reports)
                reports[i].error_pos = back[i];
            if (damaged < 0)
                damaged = (int)i;
        }
    if (damaged >= 0)
        return set_error(V1C_E_CORRUPT, "v1c_jpeg_compose: the entropy-coded data of source " + std::to_string(damaged) + " is damaged at bit " +
                                            std::to_string(back[damaged]) + " of the unstuffed scan");
    if (back[V1C_JPEG_XF_MAX_SOURCES] != 0)
        return set_error(V1C_E_UNSUPPORTED, "v1c_jpeg_compose: a coefficient outside what 8-bit samples give (AC beyond +-1023 or DC outside "
                                            "-1024 ... 1023): the encoder's tables do not code it");

    // the encoder's chain and its two synchronisations
    std::vector<uint8_t> got(back_bytes, 0);
    e = jpegxc::launch_encode_coef(b, nslots ? &o : nullptr, first, st);
    if (e == hipSuccess)
        e = hipMemcpyAsync(got.data(), b.sizes, back_bytes, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);  // 1: the sizes and the records
    if (e == hipSuccess)
        e = es;
    if (e != hipSuccess)
        return set_error(V1C_E_HIP, std::string("v1c_jpeg_compose (encode): ") + hipGetErrorString(e));
    const uint64_t* sizes = (const uint64_t*)got.data();
    for (uint32_t f = 0; f < un; f++)
        if (sizes[f] == 0 || sizes[f] > jpeg::scan_bound(im[f].g))
            return set_error(V1C_E_HIP, "v1c_jpeg_compose: internal size estimate exceeded");
    for (uint32_t f = 0; f < un && e == hipSuccess; f++)
        e = hipMemcpyAsync(outputs[f].out_host, b.buf.out + im[f].out0, sizes[f], hipMemcpyDeviceToHost, st);
    const hipError_t ec = hipStreamSynchronize(st);  // 2: the scans
    if (e == hipSuccess)
        e = ec;
    if (e != hipSuccess)
        return set_error(V1C_E_HIP, std::string("v1c_jpeg_compose (copy): ") + hipGetErrorString(e));
    for (uint32_t f = 0; f < un; f++) {
        outputs[f].size = sizes[f];
        if (slot_of[f] >= 0)
            outputs[f].dht_size = jpeg::dht_body(((const jpeg::DhtRecord*)(got.data() + (o_rec - o_sizes)))[slot_of[f]], outputs[f].dht);
    }
    return V1C_OK;
}
