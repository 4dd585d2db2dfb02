// jpegxf.hip -- host side of the lossless JPEG composer's entry points of the C ABI (v1c_jpeg_compose*, v1c_jpeg_header_xf,
// include/vr180_remap.h): the parse of every source and the rules of the outputs, all before the device is touched; then the lossless
// entries' one chain (jpegx_chain.hpp) over the sources, with this entry's gather, which takes an output's blocks from up to four
// coefficient stores and transforms them on the way.  INTEGRATION.md section 10 has the contract, DESIGN.md section 20 the design.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/vr180_remap.h"
#include "host_util.hpp"
#include "jpegx_chain.hpp"
#include "jpegxf_host.hpp"
#include "jpegxf_launch.hpp"

using namespace v1c;
using namespace v1c::jpegxf;
using jpegx::file_error;

namespace {

// what the host-only checks of a call give: the parses, and every output's geometry and regions
struct Checked {
    std::vector<jpegdec::Parsed> ps;
    std::vector<jpeg::Geom> geoms;
    std::vector<RegionList> lists;
};

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
    if (dht && (dht_size > V1C_JPEG_DHT_MAX || !jpeg::whole_tables(dht, dht_size, ps.g.nc)))
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
    const bool counted = nsources >= 1 && nsources <= V1C_JPEG_XF_MAX_SOURCES;
    if (reports && counted)
        std::memset(reports, 0, sizeof(*reports) * (size_t)nsources);
    const uint32_t S = jpegdec::subseq_of(subseq_bits);
    if (!S)
        return set_error(V1C_E_INVALID, std::string("v1c_jpeg_compose: ") + jpegdec::kSubseqRule);
    Checked c;
    std::string why;
    const int bad = call_error(nsources, sources, n, outputs, true, c, why);
    if (bad != V1C_OK) {
        if (reports && counted)
            for (size_t i = 0; i < c.ps.size(); i++)
                reports[i].error_pos = c.ps[i].error_pos;
        return set_error(bad, "v1c_jpeg_compose: " + why);
    }
    std::vector<jpegx::Source> src;
    for (int i = 0; i < nsources; i++)
        src.push_back(jpegx::Source{&c.ps[(size_t)i], sources[i].file});
    std::vector<jpegx::Output> out;
    for (int i = 0; i < n; i++) {
        const Region& r0 = c.lists[(size_t)i].r[0];  // (whose tables are every region's: check_output)
        out.push_back(jpegx::output_of(outputs[i], c.geoms[(size_t)i], c.ps[r0.source], (r0.code & kTranspose) != 0));
    }
    const jpegx::Gather gather = [&c](uint32_t f, const std::vector<jpegdec::Args>& dec, int16_t* dst, uint32_t* flag, hipStream_t st) {
        GatherArgs ga{};
        for (size_t i = 0; i < dec.size(); i++)
            ga.src[i].coef = dec[i].coef, ga.src[i].dcoff = dec[i].dcoff, ga.src[i].g = c.ps[i].g;
        ga.dst = dst, ga.dst_mcux = c.geoms[f].mcux, ga.dst_nblocks = c.geoms[f].nblocks;
        ga.flag = flag, ga.regions = c.lists[f];
        return launch_gather(ga, st);
    };
    return jpegx::run("v1c_jpeg_compose", true, device, stream, src, S, out, gather, reports);
}
