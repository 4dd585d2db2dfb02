// jpegxc.hip -- host side of the lossless JPEG transcoder's entry points of the C ABI (v1c_jpeg_transcode*, v1c_jpeg_header_xc,
// include/vr180_remap.h): the parse and the rules of the outputs, all before the device is touched; then the lossless entries' one
// chain (jpegx_chain.hpp) over the one source, with this entry's gather.  The outputs of a call are the images of one encoder chunk.
// INTEGRATION.md section 9 has the contract, DESIGN.md section 19 the design.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/vr180_remap.h"
#include "host_util.hpp"
#include "jpegx_chain.hpp"
#include "jpegxc_host.hpp"
#include "jpegxc_launch.hpp"

using namespace v1c;
using namespace v1c::jpegxc;
using jpegx::file_error;

namespace {

// what the host-only checks of a call give: the parse, and every output's geometry and regions
struct Checked {
    jpegdec::Parsed ps;
    std::vector<jpeg::Geom> geoms;
    std::vector<RegionList> lists;
};

// every check that needs no device; buffers: whether out_host and capacity count
int call_error(const uint8_t* file, uint64_t size, int n, const v1c_jpeg_xc_output* outputs, bool buffers, Checked& c, std::string& why)
{
    if (!outputs || n < 1 || n > V1C_JPEG_XC_MAX_OUTPUTS)
        return why = "1 ... " + std::to_string(V1C_JPEG_XC_MAX_OUTPUTS) + " outputs", V1C_E_INVALID;
    const int bad = file_error(file, size, c.ps, why);
    if (bad != V1C_OK)
        return bad;
    c.geoms.resize((size_t)n), c.lists.resize((size_t)n);
    for (int i = 0; i < n; i++) {
        std::string w;
        const int rc = check_output(c.ps.g, outputs[i], c.geoms[i], c.lists[i], w);
        if (rc != V1C_OK)
            return why = "output " + std::to_string(i) + ": " + w, rc;
        if (buffers && (!outputs[i].out_host || outputs[i].capacity < jpeg::scan_bound(c.geoms[i])))
            return why = "output " + std::to_string(i) + ": NULL out_host, or capacity below v1c_jpeg_transcode_bound = " +
                         std::to_string(jpeg::scan_bound(c.geoms[i])),
                   V1C_E_INVALID;
    }
    return V1C_OK;
}

}  // namespace

extern "C" uint64_t v1c_jpeg_transcode_bound(const uint8_t* file, uint64_t size, int width, int height, int restart_mcus)
{
    jpegdec::Parsed ps;
    std::string why;
    jpeg::Geom g;
    if (file_error(file, size, ps, why) != V1C_OK || !out_geom(ps.g, width, height, restart_mcus, g))
        return 0;
    return jpeg::scan_bound(g);
}

extern "C" int v1c_jpeg_transcode_check(const uint8_t* file, uint64_t size, int n, const v1c_jpeg_xc_output* outputs, uint64_t* error_pos)
{
    Checked c;
    std::string why;
    const int bad = call_error(file, size, n, outputs, false, c, why);
    if (error_pos)
        *error_pos = c.ps.error_pos;
    return bad == V1C_OK ? V1C_OK : set_error(bad, "v1c_jpeg_transcode_check: " + why);
}

extern "C" int64_t v1c_jpeg_header_xc(const uint8_t* file, uint64_t size, int width, int height, int restart_mcus, const uint8_t* dht,
                                      uint32_t dht_size, uint8_t* out, uint64_t capacity)
{
    jpegdec::Parsed ps;
    std::string why;
    const int bad = file_error(file, size, ps, why);
    if (bad != V1C_OK)
        return set_error(bad, "v1c_jpeg_header_xc: " + why);
    jpeg::Geom g;
    if (!out || !out_geom(ps.g, width, height, restart_mcus, g))
        return set_error(V1C_E_INVALID, "v1c_jpeg_header_xc: NULL pointer, or sizes or restart_mcus out of range");
    if (dht && (dht_size > V1C_JPEG_DHT_MAX || !jpeg::whole_tables(dht, dht_size, ps.g.nc)))
        return set_error(V1C_E_INVALID, "v1c_jpeg_header_xc: dht is not the tables of an optimising transcode of such a file");
    const std::vector<uint8_t> head = xc_header(ps, g, restart_mcus, dht, dht_size);
    if (capacity < head.size())
        return set_error(V1C_E_INVALID, "v1c_jpeg_header_xc: capacity is below V1C_JPEG_HEADER_XC_MAX");
    std::memcpy(out, head.data(), head.size());
    return (int64_t)head.size();
}

extern "C" int v1c_jpeg_transcode(int device, void* stream, const uint8_t* file, uint64_t size, int n, v1c_jpeg_xc_output* outputs,
                                  uint32_t subseq_bits, v1c_jpeg_decode_report* report)
{
    if (report)
        std::memset(report, 0, sizeof(*report));
    const uint32_t S = jpegdec::subseq_of(subseq_bits);
    if (!S)
        return set_error(V1C_E_INVALID, std::string("v1c_jpeg_transcode: ") + jpegdec::kSubseqRule);
    Checked c;
    std::string why;
    const int bad = call_error(file, size, n, outputs, true, c, why);
    if (bad != V1C_OK) {
        if (report)
            report->error_pos = c.ps.error_pos;
        return set_error(bad, "v1c_jpeg_transcode: " + why);
    }
    std::vector<jpegx::Output> out;
    for (int i = 0; i < n; i++)
        out.push_back(jpegx::output_of(outputs[i], c.geoms[(size_t)i], c.ps, false));
    const jpegx::Gather gather = [&c](uint32_t f, const std::vector<jpegdec::Args>& dec, int16_t* dst, uint32_t* flag, hipStream_t st) {
        GatherArgs ga{};
        ga.src = dec[0].coef, ga.dcoff = dec[0].dcoff, ga.sg = c.ps.g;
        ga.dst = dst, ga.dst_mcux = c.geoms[f].mcux, ga.dst_nblocks = c.geoms[f].nblocks;
        ga.flag = flag, ga.regions = c.lists[f];
        return launch_gather(ga, st);
    };
    return jpegx::run("v1c_jpeg_transcode", false, device, stream, {jpegx::Source{&c.ps, file}}, S, out, gather, report);
}
