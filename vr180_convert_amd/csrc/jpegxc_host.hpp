// jpegxc_host.hpp -- host side of the lossless JPEG transcoder: what a parsed file is refused for, the geometry of an output as the
// encoder's stages read it, the rules of an output's regions, and the header segments of an output -- the FILE's quantisation tables
// and sampling factors around the encoder's Huffman tables.  Everything a call can be refused for is found here, before the device is
// touched.  Shared by jpegxc.hip and the host harness (tests/host_jpegxc/jpegxc_emul.hip); tests/jpgxc_ref.py restates it.
#pragma once

#include <cstring>
#include <string>
#include <vector>

#include "../../include/vr180_remap.h"
#include "jpeg_host.hpp"
#include "jpegdec_host.hpp"
#include "jpegxc_core.hpp"

namespace v1c {
namespace jpegxc {

// Whether the file's blocks can be written again: the encoder writes two classes of tables, luminance and chrominance.  V1C_OK, or
// V1C_E_UNSUPPORTED and why.
inline int source_error(const jpegdec::Parsed& ps, std::string& why)
{
    const jpegdec::Geom& g = ps.g;
    if (g.nc == 3 && std::memcmp(ps.tab.q[g.tq[1]], ps.tab.q[g.tq[2]], sizeof(ps.tab.q[0])) != 0)
        return why = "Cb and Cr have quantisation tables of their own: more than the two classes the encoder writes", V1C_E_UNSUPPORTED;
    return V1C_OK;
}

// the geometry of a width x height output of a file of geometry s, with restart_mcus MCUs per interval (0: one interval, no DRI)
inline bool out_geom(const jpegdec::Geom& s, int width, int height, int restart_mcus, jpeg::Geom& g)
{
    if (width < 1 || height < 1 || width > 65535 || height > 65535 || restart_mcus < 0 || restart_mcus > 65535)
        return false;
    std::memset(&g, 0, sizeof(g));
    g.h = (uint32_t)height, g.w = (uint32_t)width, g.cn = g.nc = s.nc;
    g.sub = (s.hs == 2 && s.vs == 2) ? 1u : 0u;
    g.bpm = s.bpm;
    g.mcux = (g.w + 8 * s.hs - 1) / (8 * s.hs), g.mcuy = (g.h + 8 * s.vs - 1) / (8 * s.vs);
    g.nmcu = g.mcux * g.mcuy;
    g.restart = restart_mcus ? (uint32_t)restart_mcus : g.nmcu;
    g.nint = (g.nmcu + g.restart - 1) / g.restart;
    g.nblocks = g.nmcu * g.bpm;
    g.ibl = g.restart * g.bpm;
    return true;
}

// The rules of one output: its size, its restart interval, and regions that lie inside the source, inside the output, do not overlap
// there and leave no MCU of it uncovered.  The output's MCU columns and rows are those of its pixel size, so the size lies within
// (n - 1) * mcu + 1 ... n * mcu of what the regions cover exactly when they tile it.  V1C_OK with g and l, or the code and why:
// V1C_E_UNSUPPORTED for overlapping regions, V1C_E_INVALID for everything else.
inline int check_output(const jpegdec::Geom& s, const v1c_jpeg_xc_output& o, jpeg::Geom& g, RegionList& l, std::string& why)
{
    if (!out_geom(s, o.width, o.height, o.restart_mcus, g))
        return why = "width and height must be 1 ... 65535, restart_mcus 0 ... 65535", V1C_E_INVALID;
    if (o.nregions < 1 || (uint32_t)o.nregions > kMaxRegions || !o.regions)
        return why = "an output has 1 ... " + std::to_string(kMaxRegions) + " regions", V1C_E_INVALID;
    l.n = (uint32_t)o.nregions;
    uint64_t area = 0;
    for (uint32_t i = 0; i < l.n; i++) {
        const v1c_jpeg_xc_region& r = o.regions[i];
        if (r.src_x < 0 || r.src_y < 0 || r.nx < 1 || r.ny < 1 || r.dst_x < 0 || r.dst_y < 0)
            return why = "region " + std::to_string(i) + ": negative origin or empty", V1C_E_INVALID;
        if ((uint64_t)r.src_x + (uint64_t)r.nx > s.mcux || (uint64_t)r.src_y + (uint64_t)r.ny > s.mcuy)
            return why = "region " + std::to_string(i) + " leaves the source's " + std::to_string(s.mcux) + " x " + std::to_string(s.mcuy) + " MCUs",
                   V1C_E_INVALID;
        if ((uint64_t)r.dst_x + (uint64_t)r.nx > g.mcux || (uint64_t)r.dst_y + (uint64_t)r.ny > g.mcuy)
            return why = "region " + std::to_string(i) + " leaves the output's " + std::to_string(g.mcux) + " x " + std::to_string(g.mcuy) +
                         " MCUs: the output's size is not what the regions cover",
                   V1C_E_INVALID;
        l.r[i] = Region{(uint32_t)r.src_x, (uint32_t)r.src_y, (uint32_t)r.nx, (uint32_t)r.ny, (uint32_t)r.dst_x, (uint32_t)r.dst_y};
        area += (uint64_t)r.nx * (uint64_t)r.ny;
        for (uint32_t j = 0; j < i; j++) {
            const Region &a = l.r[i], &b = l.r[j];
            if (a.dx < b.dx + b.nx && b.dx < a.dx + a.nx && a.dy < b.dy + b.ny && b.dy < a.dy + a.ny)
                return why = "regions " + std::to_string(j) + " and " + std::to_string(i) + " overlap in the output", V1C_E_UNSUPPORTED;
        }
    }
    // (inside the output and disjoint: they cover it exactly when their areas add up to it)
    if (area != g.nmcu)
        return why = "the regions leave " + std::to_string(g.nmcu - area) + " MCUs of the output uncovered", V1C_E_INVALID;
    return V1C_OK;
}

// the body of the DHT segment with the Annex K tables: the two of one component, or the four of three
inline std::vector<uint8_t> annex_k_dht(uint32_t nc)
{
    const jpeg::HuffSpec* specs[4] = {&jpeg::kDcLuma, &jpeg::kAcLuma, &jpeg::kDcChroma, &jpeg::kAcChroma};
    const uint8_t ids[4] = {0x00, 0x10, 0x01, 0x11};
    std::vector<uint8_t> b;
    for (uint32_t i = 0; i < (nc == 1 ? 2u : 4u); i++) {
        b.push_back(ids[i]);
        b.insert(b.end(), specs[i]->bits, specs[i]->bits + 16);
        b.insert(b.end(), specs[i]->vals, specs[i]->vals + specs[i]->n);
    }
    return b;
}

using jpeg::whole_tables;  // the rule of a DHT body a caller hands back: the encoder's (jpeg_host.hpp), for the callers of this header

// SOI, APP0 (JFIF 1.01, aspect 1:1), DQT, SOF, DHT, DRI, SOS of an output of geometry g cut from the parsed file: the file's
// quantisation tables as table 0 (luminance) and table 1 (chrominance), its sampling factors, the DHT body `dht` (NULL: the Annex K
// tables) and DRI unless restart_mcus is 0.  Entries above 255 make the tables 16-bit and the frame SOF1, as the standard asks.  The
// source's APPn and COM segments are not carried over.
inline std::vector<uint8_t> xc_header(const jpegdec::Parsed& ps, const jpeg::Geom& g, int restart_mcus, const uint8_t* dht = nullptr,
                                      uint32_t dht_size = 0)
{
    using jpeg::put_segment;
    const jpegdec::Geom& s = ps.g;
    const uint32_t ntab = s.nc == 1 ? 1u : 2u;
    bool wide = false;
    for (uint32_t i = 0; i < ntab; i++)
        for (int n = 0; n < 64; n++)
            wide |= ps.tab.q[s.tq[i]][n] > 255;
    std::vector<uint8_t> out = {0xff, 0xd8};
    put_segment(out, 0xe0, {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    std::vector<uint8_t> b;
    for (uint32_t i = 0; i < ntab; i++) {
        b.push_back((uint8_t)((wide ? 0x10 : 0) | i));
        const size_t at = b.size();
        b.resize(at + (wide ? 128 : 64));
        for (int n = 0; n < 64; n++) {
            const uint16_t v = ps.tab.q[s.tq[i]][n];
            const int k = jpeg::zigzag_of(n);
            if (wide)
                b[at + 2 * k] = (uint8_t)(v >> 8), b[at + 2 * k + 1] = (uint8_t)v;
            else
                b[at + k] = (uint8_t)v;
        }
    }
    put_segment(out, 0xdb, b);
    b = {8, (uint8_t)(g.h >> 8), (uint8_t)g.h, (uint8_t)(g.w >> 8), (uint8_t)g.w, (uint8_t)s.nc};
    for (uint32_t i = 0; i < s.nc; i++)
        b.insert(b.end(), {(uint8_t)(i + 1), (uint8_t)(i == 0 && s.nc == 3 ? (s.hs << 4 | s.vs) : 0x11), (uint8_t)(i ? 1 : 0)});
    put_segment(out, wide ? 0xc1 : 0xc0, b);
    if (dht)
        b.assign(dht, dht + dht_size);
    else
        b = annex_k_dht(s.nc);
    put_segment(out, 0xc4, b);
    if (restart_mcus)
        put_segment(out, 0xdd, {(uint8_t)(restart_mcus >> 8), (uint8_t)restart_mcus});
    b = {(uint8_t)s.nc};
    for (uint32_t i = 0; i < s.nc; i++)
        b.insert(b.end(), {(uint8_t)(i + 1), (uint8_t)(i ? 0x11 : 0x00)});
    b.insert(b.end(), {0, 63, 0});
    put_segment(out, 0xda, b);
    return out;
}

}  // namespace jpegxc
}  // namespace v1c
