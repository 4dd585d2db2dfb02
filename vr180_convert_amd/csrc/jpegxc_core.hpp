// jpegxc_core.hpp -- per-block arithmetic of the lossless JPEG transcoder (kernels_jpegxc.hip, jpegxc.hip): which block of the source
// file a block of an output is, the value of that block's DC, and whether a coefficient is one the encoder's tables can code.  A
// transcode cuts a file on MCU boundaries: an output is tiled by regions, rectangles of source MCUs placed at a destination MCU, and
// every coefficient of every block is carried over as it is.
//
// __host__ __device__ so that tests/host_jpegxc/jpegxc_emul.hip runs exactly this code on the host against the restatement
// (tests/jpgxc_ref.py).  INTEGRATION.md section 9 has the contract.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jpeg_core.hpp"
#include "jpegdec_core.hpp"

namespace v1c {
namespace jpegxc {

constexpr uint32_t kMaxRegions = 16;          // of one output: crop has one, swap two
constexpr uint32_t kNone = 0xffffffffu;       // no source: the destination MCU lies in no region

// a rectangle of nx x ny source MCUs from (sx, sy), placed with its first MCU at (dx, dy) of the output
struct Region {
    uint32_t sx, sy, nx, ny, dx, dy;
};

struct RegionList {
    uint32_t n;
    Region r[kMaxRegions];
};

// the source MCU of the output's MCU (mx, my); regions do not overlap in the destination (jpegxc_host.hpp: check_output), so at most
// one holds it.  (mx - r.dx wraps to a large number left of the region: one comparison per axis)
__host__ __device__ inline uint32_t source_mcu(const RegionList& l, uint32_t src_mcux, uint32_t mx, uint32_t my)
{
    uint32_t s = kNone;
    for (uint32_t i = 0; i < l.n && i < kMaxRegions; i++) {
        const Region& r = l.r[i];
        if (mx - r.dx < r.nx && my - r.dy < r.ny)
            s = (r.sy + (my - r.dy)) * src_mcux + r.sx + (mx - r.dx);
    }
    return s;
}

// the source block of block b of an output that is dst_mcux MCUs wide: the same block of the MCU, bpm blocks each
__host__ __device__ inline uint32_t source_block(const RegionList& l, uint32_t src_mcux, uint32_t dst_mcux, uint32_t bpm, uint32_t b)
{
    const uint32_t mcu = b / bpm, k = b - mcu * bpm;
    const uint32_t my = mcu / dst_mcux, mx = mcu - my * dst_mcux;
    const uint32_t s = source_mcu(l, src_mcux, mx, my);
    return s == kNone ? kNone : s * bpm + k;
}

// The DC of source block sb as a value.  The decoder's last pass leaves the DC DIFFERENCE in coefficient 0 (jpegdec_core.hpp:
// decode_span); the differences ordered by component are summed by a scan (dcoff: its exclusive sums, modulo 2^32 is what counts), and
// the value is the inclusive sum at the block minus the exclusive sum at its segment's first block of the component -- what the
// decoder's inverse DCT computes for itself (jpegdec_kernels.hpp: idct_body), but NOT cut to 16 bits: a sum that passes 16 bits must
// be seen as out of range (codable), not wrap into it.  The coefficient stored is the value's low 16 bits.
__host__ __device__ inline int dc_value(const jpegdec::Geom& g, const uint64_t* dcoff, uint32_t sb)
{
    uint32_t at, at0;
    jpegdec::dc_pos(g, sb, at, at0);
    return (int)(uint32_t)(dcoff[at + 1] - dcoff[at0]);
}

// Whether the encoder's tables code the coefficient wherever the cut puts it: an AC coefficient of category 10 at the most, a DC
// within [-1024, 1023], so that the difference of ANY two is of category 11 at the most.  Every file of 8-bit samples is inside (a DC
// is the block's level-shifted sum / 8 / q: -1024 ... 1016); files of valid syntax and absurd numbers are not, and are refused.
__host__ __device__ inline bool codable(int v, bool dc)
{
    return dc ? (v >= -1024 && v <= 1023) : (v >= -1023 && v <= 1023);
}

// ---- the output's blocks as the entropy coder sees them ----------------------------------------------------------------------------------
// The encoder's own geometry helpers (jpeg_core.hpp: block_pos, dc_predecessor) know MCUs of one block per component and of four luma
// blocks; a transcoded 4:2:2 file has two.  These two say the same for ANY number of luma blocks: an output's Geom has nc components
// and bpm blocks per MCU, of which all but the last nc - 1 are luma.

// luma blocks of an MCU
__host__ __device__ inline uint32_t luma_blocks(const jpeg::Geom& g)
{
    return g.bpm - (g.nc - 1);
}

// the table class of block b: 0 luminance, 1 chrominance
__host__ __device__ inline int table_class(const jpeg::Geom& g, uint32_t b)
{
    return b % g.bpm < luma_blocks(g) ? 0 : 1;
}

// the block whose DC the difference of block b is taken against, or b itself where the prediction is 0 (an interval's first block of
// each component): the luma block in front within the MCU, else the last luma block of the MCU in front; for chroma the same block
// of the MCU in front
__host__ __device__ inline uint32_t xc_predecessor(const jpeg::Geom& g, uint32_t b)
{
    const uint32_t mcu = b / g.bpm, k = b - mcu * g.bpm, ny = luma_blocks(g);
    if (k >= 1 && k < ny)
        return b - 1;
    if (mcu % g.restart == 0)
        return b;
    return k == 0 ? b - g.bpm + ny - 1 : b - g.bpm;
}

// the DC block b of an output whose blocks start at block blk0 of `coef` is predicted from
__host__ __device__ inline int xc_prediction(const jpeg::Geom& g, const int16_t* coef, uint64_t blk0, uint32_t b)
{
    const uint32_t p = xc_predecessor(g, b);
    return p == b ? 0 : coef[(size_t)(blk0 + p) * 64];
}

}  // namespace jpegxc
}  // namespace v1c
