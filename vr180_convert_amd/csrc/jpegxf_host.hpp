// jpegxf_host.hpp -- host side of the lossless JPEG composer: what a set of parsed files is refused for, the rules of an output's
// regions with their transforms, and the header segments of an output -- the quantisation tables of its first region's file,
// transposed where that region transposes.  Everything a call can be refused for is found here, before the device is touched.  The
// single file's rules, the output's geometry and the header writer are the transcoder's (jpegxc_host.hpp).  Shared by jpegxf.hip and
// the host harness (tests/host_jpegxf/jpegxf_emul.hip); tests/jpgxf_ref.py restates it.
#pragma once

#include <cstring>
#include <string>
#include <vector>

#include "../../include/vr180_remap.h"
#include "jpegxc_host.hpp"
#include "jpegxf_core.hpp"

namespace v1c {
namespace jpegxf {

// Whether the files can be composed: each one a file the transcoder takes, all of the first one's component count and sampling
// factors.  V1C_OK, or V1C_E_UNSUPPORTED and why.
inline int sources_error(const std::vector<jpegdec::Parsed>& ps, std::string& why)
{
    for (size_t i = 0; i < ps.size(); i++) {
        const int bad = jpegxc::source_error(ps[i], why);
        if (bad != V1C_OK)
            return why = "source " + std::to_string(i) + ": " + why, bad;
        const jpegdec::Geom &a = ps[0].g, &b = ps[i].g;
        if (a.nc != b.nc || a.hs != b.hs || a.vs != b.vs)
            return why = "source " + std::to_string(i) + " has other components or sampling factors than source 0", V1C_E_UNSUPPORTED;
    }
    return V1C_OK;
}

// The quantisation tables a region's blocks are to be read with, luminance and chrominance, row-major: the file's, transposed where
// the region transposes
inline void effective_tables(const jpegdec::Parsed& ps, bool transposed, uint16_t q[2][64])
{
    const jpegdec::Geom& s = ps.g;
    for (int t = 0; t < 2; t++)
        for (int n = 0; n < 64; n++)
            q[t][n] = ps.tab.q[s.tq[s.nc == 3 ? t : 0]][transposed ? ((n & 7) << 3 | n >> 3) : n];
}

// the parse of a file with its quantisation tables transposed: what the transcoder's header writer takes for a transposing output
inline jpegdec::Parsed transposed_tables(const jpegdec::Parsed& ps)
{
    jpegdec::Parsed out = ps;
    for (int t = 0; t < 4; t++)
        for (int n = 0; n < 64; n++)
            out.tab.q[t][n] = ps.tab.q[t][(n & 7) << 3 | n >> 3];
    return out;
}

// The rules of one output over the parsed files ps (sources_error passed): its size and restart interval (jpegxc_host.hpp:
// out_geom), regions that name a source and a transform, lie inside their source and -- as the NX x NY MCUs they are placed as --
// inside the output, do not overlap there and leave no MCU of it uncovered; no transposing code where hs != vs; and every region's
// effective quantisation tables those of region 0.  V1C_OK with g and l, or the code and why: V1C_E_UNSUPPORTED for overlapping
// regions, a transposed 4:2:2 file and unequal tables, V1C_E_INVALID for everything else.
inline int check_output(const std::vector<jpegdec::Parsed>& ps, const v1c_jpeg_xf_output& o, jpeg::Geom& g, RegionList& l, std::string& why)
{
    const jpegdec::Geom& s0 = ps[0].g;
    if (!jpegxc::out_geom(s0, o.width, o.height, o.restart_mcus, g))
        return why = "width and height must be 1 ... 65535, restart_mcus 0 ... 65535", V1C_E_INVALID;
    if (o.nregions < 1 || (uint32_t)o.nregions > kMaxRegions || !o.regions)
        return why = "an output has 1 ... " + std::to_string(kMaxRegions) + " regions", V1C_E_INVALID;
    l.n = (uint32_t)o.nregions;
    uint64_t area = 0;
    uint16_t q0[2][64], q[2][64];
    for (uint32_t i = 0; i < l.n; i++) {
        const v1c_jpeg_xf_region& r = o.regions[i];
        const std::string name = "region " + std::to_string(i);
        if (r.source < 0 || (size_t)r.source >= ps.size() || r.transform < 0 || r.transform > 7)
            return why = name + ": no such source, or a transform outside 0 ... 7", V1C_E_INVALID;
        const jpegdec::Geom& s = ps[(size_t)r.source].g;
        if (r.src_x < 0 || r.src_y < 0 || r.nx < 1 || r.ny < 1 || r.dst_x < 0 || r.dst_y < 0)
            return why = name + ": negative origin or empty", V1C_E_INVALID;
        if ((uint64_t)r.src_x + (uint64_t)r.nx > s.mcux || (uint64_t)r.src_y + (uint64_t)r.ny > s.mcuy)
            return why = name + " leaves its source's " + std::to_string(s.mcux) + " x " + std::to_string(s.mcuy) + " MCUs", V1C_E_INVALID;
        if (((uint32_t)r.transform & kTranspose) && s.hs != s.vs)
            return why = name + ": a transposed 4:2:2 file would be 4:4:0, which neither codec handles", V1C_E_UNSUPPORTED;
        l.r[i] = Region{(uint32_t)r.source, (uint32_t)r.transform, (uint32_t)r.src_x, (uint32_t)r.src_y, (uint32_t)r.nx, (uint32_t)r.ny,
                        (uint32_t)r.dst_x, (uint32_t)r.dst_y, s.mcux};
        const uint64_t NX = placed_nx(l.r[i]), NY = placed_ny(l.r[i]);
        if ((uint64_t)r.dst_x + NX > g.mcux || (uint64_t)r.dst_y + NY > g.mcuy)
            return why = name + " leaves the output's " + std::to_string(g.mcux) + " x " + std::to_string(g.mcuy) +
                         " MCUs: the output's size is not what the regions cover",
                   V1C_E_INVALID;
        area += NX * NY;
        for (uint32_t j = 0; j < i; j++) {
            const Region &a = l.r[i], &b = l.r[j];
            if (a.dx < b.dx + placed_nx(b) && b.dx < a.dx + placed_nx(a) && a.dy < b.dy + placed_ny(b) && b.dy < a.dy + placed_ny(a))
                return why = "regions " + std::to_string(j) + " and " + std::to_string(i) + " overlap in the output", V1C_E_UNSUPPORTED;
        }
        effective_tables(ps[(size_t)r.source], ((uint32_t)r.transform & kTranspose) != 0, i ? q : q0);
        if (i && std::memcmp(q, q0, sizeof(q)) != 0)
            return why = name + ": its quantisation tables, transposed where it transposes, are not region 0's", V1C_E_UNSUPPORTED;
    }
    // (inside the output and disjoint: they cover it exactly when their areas add up to it)
    if (area != g.nmcu)
        return why = "the regions leave " + std::to_string(g.nmcu - area) + " MCUs of the output uncovered", V1C_E_INVALID;
    return V1C_OK;
}

// the header segments of an output (jpegxc_host.hpp: xc_header) with the file's quantisation tables transposed where `transposed`
inline std::vector<uint8_t> xf_header(const jpegdec::Parsed& ps, bool transposed, const jpeg::Geom& g, int restart_mcus, const uint8_t* dht = nullptr,
                                      uint32_t dht_size = 0)
{
    return transposed ? jpegxc::xc_header(transposed_tables(ps), g, restart_mcus, dht, dht_size) : jpegxc::xc_header(ps, g, restart_mcus, dht, dht_size);
}

}  // namespace jpegxf
}  // namespace v1c
