// jpegx_chain.hpp -- the one host chain of the lossless JPEG entries (v1c_jpeg_transcode: jpegxc.hip; v1c_jpeg_compose: jpegxf.hip),
// from the device of a call to its return: every source's decode in turn up to its DC scan, each into a coefficient store of its
// own (jpegdec_launch.hpp: decode_to_coef, with the rounds the host reads a flag between), the gather of every output from those
// stores, one synchronisation for every verdict, and one chunk of the batch encoder from a filled coefficient store on
// (jpegxc_launch.hpp: launch_encode_coef; jpeg_chunk.hpp: its layout and its end with two synchronisations).  A transcode is a
// composition of one source: the entries differ in their host-only checks, in the gather kernel they launch, and in a few words of
// the messages.  Host code only.
#pragma once

#include <hip/hip_runtime.h>

#include <functional>
#include <string>
#include <vector>

#include "../../include/vr180_remap.h"
#include "host_util.hpp"
#include "jpeg_chunk.hpp"
#include "jpeg_host.hpp"
#include "jpegxc_launch.hpp"
#include "jpegxf_host.hpp"

namespace v1c {
namespace jpegx {

// the parse of one source and its scope: V1C_OK, or the code and why
inline int file_error(const uint8_t* file, uint64_t size, jpegdec::Parsed& ps, std::string& why)
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

// The tables an output's stages read: the Annex K codes (an optimising output's are overwritten on the device); the quantiser half,
// which no stage behind the transform reads, is that of the output's header
inline void make_tables(const jpegdec::Parsed& ps, bool transposed, jpeg::Tables& t)
{
    jpegxf::effective_tables(ps, transposed, t.q);
    jpeg::code_table(jpeg::kDcLuma, t.dc[0], 16);
    jpeg::code_table(jpeg::kDcChroma, t.dc[1], 16);
    jpeg::code_table(jpeg::kAcLuma, t.ac[0], 256);
    jpeg::code_table(jpeg::kAcChroma, t.ac[1], 256);
}

struct Source {
    const jpegdec::Parsed* ps;
    const uint8_t* file;
};

// One output as the chain sees it, whichever entry's struct it came in: its geometry, its Tables, and where its results go
struct Output {
    jpeg::Geom g;
    jpeg::Tables tab;
    bool optimize;
    jpeg::Result to;
};

// o: a v1c_jpeg_xc_output or a v1c_jpeg_xf_output of geometry g; ps, transposed: whose quantiser tables its header has
template <class CallerOutput>
inline Output output_of(CallerOutput& o, const jpeg::Geom& g, const jpegdec::Parsed& ps, bool transposed)
{
    Output x;
    x.g = g, x.optimize = o.optimize != 0;
    make_tables(ps, transposed, x.tab);
    x.to = jpeg::Result{o.out_host, &o.size, o.dht, &o.dht_size};
    return x;
}

// launches output f's gather from the decoders' stores into dst, its blocks in the encoder's store; flag: the range flag
using Gather = std::function<hipError_t(uint32_t f, const std::vector<jpegdec::Args>& dec, int16_t* dst, uint32_t* flag, hipStream_t st)>;

// A checked call.  name: the entry, for the messages, which count the sources where name_source; S: the bits of a subsequence;
// reports: one per source, or NULL.
inline int run(const std::string& name, bool name_source, int device, void* stream, const std::vector<Source>& src, uint32_t S,
               const std::vector<Output>& out, const Gather& gather, v1c_jpeg_decode_report* reports)
{
    using jpeg::Image;
    using jpeg::Tables;
    if (device < 0 || device >= kMaxDevices)
        return set_error(V1C_E_NODEVICE, name + ": no such device");
    DeviceGuard dg(device);
    if (!dg.ok)
        return set_error(V1C_E_NODEVICE, "hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    if (stream_is_capturing(st))
        return set_error(V1C_E_UNSUPPORTED, name + ": the host reads a flag between the rounds and the sizes between the kernels and the "
                                                   "copies, so the call cannot be captured into a graph");
    for (const Output& o : out)
        *o.to.size = 0, *o.to.dht_size = 0;

    // the decoders' parts of the workspace, one per source: its upload, and its work up to the planes, which no pixel stage fills here
    struct Decode {
        uint32_t nsub;
        jpegdec::Layout l;
        size_t at;                   // in the workspace
        std::vector<uint8_t> stage;  // (pageable: alive until the call's last synchronisation)
    };
    const uint32_t us = (uint32_t)src.size(), un = (uint32_t)out.size();
    std::vector<Decode> dec(us);
    size_t dec_bytes = 0;
    for (uint32_t i = 0; i < us; i++) {
        const jpegdec::Parsed& ps = *src[i].ps;
        Decode& d = dec[i];
        const std::vector<uint32_t> subfirst = jpegdec::sub_first(ps, S);
        d.nsub = subfirst.back();
        if (reports)
            reports[i].segments = ps.g.nseg, reports[i].subsequences = d.nsub;
        d.l = jpegdec::layout_of(ps, d.nsub);
        d.at = dec_bytes, dec_bytes += align256(d.l.up_bytes + d.l.o_p0);
        d.stage.assign(d.l.up_bytes, 0);
        jpegdec::stage_file(d.stage.data(), ps, d.l, subfirst, src[i].file);
    }

    // the encoder's part, as a chunk of v1c_jpeg_encode_batch_opt lays it out (jpeg_chunk.hpp), with one Tables per output and the
    // flag of the gathers behind the head
    std::vector<int32_t> slot_of(un, -1);
    std::vector<jpeg::OptSlot> slots;
    for (uint32_t f = 0; f < un; f++)
        if (out[f].optimize) {
            slot_of[f] = (int32_t)slots.size();
            slots.push_back(jpeg::OptSlot{f, src[0].ps->g.nc == 1 ? 2u : 4u});  // (the components are those of every source)
        }
    const size_t nslots = slots.size();
    const jpeg::HeadLayout h = jpeg::head_layout(un, un, nslots, true);
    std::vector<uint8_t> up(h.o_sizes, 0);  // (pageable, as the decoders' uploads: alive until the call's last synchronisation)
    Image* im = (Image*)(up.data() + h.o_im);
    uint32_t* first = (uint32_t*)(up.data() + h.o_first);
    for (uint32_t f = 0; f < un; f++) {
        im[f].img = nullptr, im[f].pitch = 0, im[f].g = out[f].g, im[f].tab = f;
        ((Tables*)(up.data() + h.o_tabs))[f] = out[f].tab;
    }
    const jpeg::Totals t = jpeg::place_regions(im, un, first);
    jpeg::stage_slots(up.data(), h, slot_of, slots);
    const jpeg::StageLayout sl = jpeg::stage_layout(h.bytes, t);

    Workspace ws(st);
    hipError_t e = hipMallocAsync((void**)&ws.p, dec_bytes + sl.bytes, st);
    if (e != hipSuccess)
        return set_error(V1C_E_HIP, name + ": hipMallocAsync: " + hipGetErrorString(e));
    uint8_t* enc = ws.p + dec_bytes;
    jpeg::Batch b;
    jpeg::OptBatch o;
    jpeg::chunk_args(h, enc, un, nslots, t, sl.at(enc), b, o);
    uint32_t* xflag = (uint32_t*)(enc + h.o_flag);

    e = hipMemcpyAsync(enc, up.data(), h.o_sizes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = hipMemsetAsync(b.buf.raw, 0, sl.raw_bytes, st);
    if (e == hipSuccess)
        e = hipMemsetAsync(b.sizes, 0, h.zero_bytes, st);

    // every source's decode up to the coefficients and its DC scan, in turn; what comes back meanwhile: a round's flag
    std::vector<jpegdec::Args> args(us);
    uint32_t more = 0;
    for (uint32_t i = 0; i < us && e == hipSuccess; i++) {
        const Decode& d = dec[i];
        uint8_t* base = ws.p + d.at;
        args[i] = jpegdec::args_of(*src[i].ps, d.l, d.nsub, S, base, base + d.l.up_bytes, (uint32_t*)(base + d.l.up_bytes + d.l.o_flags), nullptr, 0, 3);
        uint32_t r = 0;
        e = jpegdec::decode_to_coef(args[i], d.l, d.stage.data(), d.nsub, st, &more, &r);
        if (reports)
            reports[i].rounds = r;
        // (Unlike v1c_jpeg_decode, which reads the verdict before its pixel stage, the DC scan and the gathers are queued before the
        //  decoder's error word is read: one synchronisation brings every source's together with the gathers' range flag.  On a
        //  damaged scan they run over whatever the last pass left; that is safe -- every index comes from the geometry, never from
        //  the data, and every load stays inside the source's zeroed store -- and the encoder's chain, whose bounds do depend on the
        //  data, is launched only behind both verdicts.)
        if (e == hipSuccess)
            e = jpegxc::launch_dc(args[i], st);
    }
    for (uint32_t f = 0; f < un && e == hipSuccess; f++)
        e = gather(f, args, b.buf.coef + (size_t)im[f].blk0 * 64, xflag, st);
    // one synchronisation for every verdict: each source's error word, and the gathers' range flag
    std::vector<uint32_t> back(us + 1, 0);
    for (uint32_t i = 0; i < us && e == hipSuccess; i++)
        e = hipMemcpyAsync(&back[i], args[i].flags + 2, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess)
        e = hipMemcpyAsync(&back[us], xflag, 4, hipMemcpyDeviceToHost, st);
    const hipError_t ev = hipStreamSynchronize(st);  // (also on an error above: nothing of this call reads the host's buffers after it)
    if (e == hipSuccess)
        e = ev;
    if (e != hipSuccess)
        return set_error(V1C_E_HIP, name + " (decode): " + hipGetErrorString(e));
    int damaged = -1;
    for (uint32_t i = 0; i < us; i++)
        if (back[i] != jpegdec::kNoError) {
            if (reports)
                reports[i].error_pos = back[i];
            if (damaged < 0)
                damaged = (int)i;
        }
    if (damaged >= 0)
        return set_error(V1C_E_CORRUPT, name + ": the entropy-coded data " + (name_source ? "of source " + std::to_string(damaged) + " " : "") +
                                            "is damaged at bit " + std::to_string(back[damaged]) + " of the unstuffed scan");
    if (back[us] != 0)
        return set_error(V1C_E_UNSUPPORTED, name + ": a coefficient outside what 8-bit samples give (AC beyond +-1023 or DC outside "
                                                   "-1024 ... 1023): the encoder's tables do not code it");

    // the encoder's chain and its two synchronisations
    e = jpegxc::launch_encode_coef(b, nslots ? &o : nullptr, first, st);
    switch (jpeg::finish_chunk(b, h, im, slot_of, [&](uint32_t f) { return out[f].to; }, st, e)) {
    case jpeg::kFinishKernels:
        return set_error(V1C_E_HIP, name + " (encode): " + hipGetErrorString(e));
    case jpeg::kFinishSizes:
        return set_error(V1C_E_HIP, name + ": internal size estimate exceeded");
    case jpeg::kFinishCopy:
        return set_error(V1C_E_HIP, name + " (copy): " + hipGetErrorString(e));
    case jpeg::kFinished:
        break;
    }
    return V1C_OK;
}

}  // namespace jpegx
}  // namespace v1c
