// jpegxf_core.hpp -- per-block arithmetic of the lossless JPEG composer (kernels_jpegxf.hip, jpegxf.hip): rotation, flip and transpose
// of MCU rectangles in the DCT domain, gathered from up to four decoded files.  A transform is three bits: transpose first (bit 2), then
// mirror x (bit 0), then mirror y (bit 1).  With F[v][u] a block's coefficient of vertical frequency v and horizontal frequency u, the
// transpose gives F'[v][u] = F[u][v], mirror x then multiplies by (-1)^u and mirror y by (-1)^v; the DC never changes.  The MCUs of a
// region, and the luma blocks of an MCU on their hs x vs grid, move the same way.  Which block of which source a block of an output is,
// which coefficient of it a coefficient is and with which sign: that is all of it, and no coefficient's magnitude changes.
//
// __host__ __device__ so that tests/host_jpegxf/jpegxf_emul.hip runs exactly this code on the host against the restatement
// (tests/jpgxf_ref.py).  INTEGRATION.md section 10 has the contract.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jpegxc_core.hpp"

namespace v1c {
namespace jpegxf {

constexpr uint32_t kMaxSources = 4;
constexpr uint32_t kMaxRegions = 16;
constexpr uint32_t kNone = 0xffffffffu;

constexpr uint32_t kMirrorX = 1, kMirrorY = 2, kTranspose = 4;  // the bits of a transform's code

// nx x ny source MCUs of file `source` from (sx, sy), transformed by `code` and placed with the first MCU of the RESULT at (dx, dy);
// src_mcux: the MCUs of a row of that file
struct Region {
    uint32_t source, code, sx, sy, nx, ny, dx, dy, src_mcux;
};

struct RegionList {
    uint32_t n;
    Region r[kMaxRegions];
};

// the MCUs a region covers in the output
__host__ __device__ inline uint32_t placed_nx(const Region& r) { return (r.code & kTranspose) ? r.ny : r.nx; }
__host__ __device__ inline uint32_t placed_ny(const Region& r) { return (r.code & kTranspose) ? r.nx : r.ny; }

// ---- coefficients: the zigzag order's transpose and the sign masks -----------------------------------------------------------------------
namespace detail {

// zigzag position of a row-major index (jpeg_core.hpp: zigzag_of, as a constant expression; the host harness compares the two)
constexpr int zz(int natural)
{
    const int r = natural >> 3, c = natural & 7, s = r + c;
    const int before = s < 8 ? s * (s + 1) / 2 : 64 - (15 - s) * (16 - s) / 2;
    const int lo = s < 8 ? 0 : s - 7;
    return before + ((s & 1) ? r - lo : c - lo);
}

// the zigzag positions of the transposed places of zigzag positions 8 * part ... 8 * part + 7, eight bits each
constexpr uint64_t tz_packed(int part)
{
    uint64_t w = 0;
    for (int n = 0; n < 64; n++)
        if (zz(n) >> 3 == part)
            w |= (uint64_t)zz((n & 7) << 3 | n >> 3) << (8 * (zz(n) & 7));
    return w;
}

// the zigzag positions whose coefficient a transform negates: odd horizontal frequency under mirror x, odd vertical under mirror y
constexpr uint64_t sign_mask(uint32_t code)
{
    uint64_t m = 0;
    for (int n = 0; n < 64; n++)
        if ((((code & kMirrorX) ? n : 0) ^ ((code & kMirrorY) ? n >> 3 : 0)) & 1)
            m |= 1ull << zz(n);
    return m;
}

}  // namespace detail

// zigzag positions (eight bits each) that the transposed block's positions 8 * part ... 8 * part + 7 are read from
__host__ __device__ inline uint64_t transposed_from(uint32_t part)
{
    constexpr uint64_t k[8] = {detail::tz_packed(0), detail::tz_packed(1), detail::tz_packed(2), detail::tz_packed(3),
                               detail::tz_packed(4), detail::tz_packed(5), detail::tz_packed(6), detail::tz_packed(7)};
    return k[part & 7u];
}

// the source's zigzag position of the result's zigzag position z
__host__ __device__ inline uint32_t source_coefficient(uint32_t code, uint32_t z)
{
    return (code & kTranspose) ? (uint32_t)(transposed_from(z >> 3) >> (8 * (z & 7u))) & 0xffu : z;
}

// the RESULT's zigzag positions that are negated: a mask of 64 bits (the mirrors come after the transpose, so u and v are the result's)
__host__ __device__ inline uint64_t negated(uint32_t code)
{
    constexpr uint64_t k[4] = {detail::sign_mask(0), detail::sign_mask(1), detail::sign_mask(2), detail::sign_mask(3)};
    return k[code & 3u];
}

// ---- MCUs and blocks -------------------------------------------------------------------------------------------------------------------
struct SourceBlock {
    uint32_t source, code, block;  // block == kNone: no region holds the MCU
};

// The source block of block b of an output that is dst_mcux MCUs wide, of files with hs x vs luma blocks and bpm blocks per MCU.
// Regions do not overlap in the output (jpegxf_host.hpp: check_output), so at most one holds the MCU.  Mirror x is undone first, then
// mirror y, then the transpose; the luma blocks of the MCU go the same way on their grid (a transposing code only where hs == vs).
__host__ __device__ inline SourceBlock source_block(const RegionList& l, uint32_t dst_mcux, uint32_t hs, uint32_t vs,
                                                    uint32_t bpm, uint32_t b)
{
    const uint32_t mcu = b / bpm, k = b - mcu * bpm;
    const uint32_t my = mcu / dst_mcux, mx = mcu - my * dst_mcux;
    SourceBlock s{0, 0, kNone};
    for (uint32_t n = 0; n < l.n && n < kMaxRegions; n++) {
        const Region& r = l.r[n];
        const uint32_t NX = placed_nx(r), NY = placed_ny(r);
        uint32_t i = mx - r.dx, j = my - r.dy;  // (wraps to a large number left of the region: one comparison per axis)
        if (i >= NX || j >= NY)
            continue;
        uint32_t bx = k % hs, by = k / hs;      // (of a luma block; a chroma block stays where it is)
        if (r.code & kMirrorX)
            i = NX - 1 - i, bx = hs - 1 - bx;
        if (r.code & kMirrorY)
            j = NY - 1 - j, by = vs - 1 - by;
        if (r.code & kTranspose) {
            uint32_t t = i;
            i = j, j = t;
            t = bx, bx = by, by = t;
        }
        const uint32_t sk = k < hs * vs ? by * hs + bx : k;
        s.source = r.source, s.code = r.code;
        s.block = ((r.sy + j) * r.src_mcux + r.sx + i) * bpm + sk;
    }
    return s;
}

}  // namespace jpegxf
}  // namespace v1c
