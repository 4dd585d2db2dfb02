// jpeg_core.hpp -- per-sample and per-block arithmetic of the device JPEG encoder (kernels_jpeg.hip, jpeg.hip): geometry, colour
// conversion, chroma downsampling, the integer forward DCT, quantisation and the entropy coder of one block.
//
// __host__ __device__ so that tests/host_jpeg/jpeg_emul.hip runs exactly this code on the host against the NumPy restatement
// (tests/jpg_ref.py).  Integer arithmetic throughout: the file is a pure function of the pixels and the parameters
// (INTEGRATION.md section 7).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace v1c {
namespace jpeg {

constexpr int kSub444 = 0, kSub420 = 2;           // V1C_JPEG_444 / V1C_JPEG_420
constexpr int kMaxBlockBits = 22 + 63 * 26;       // the longest DC token (chrominance, category 11) and 63 times the longest AC token
constexpr int kMaxBlockBytes = (kMaxBlockBits + 7) / 8;
constexpr int kPiece = 16;                        // bytes of the unstuffed stream one lane of the stuffing kernels takes

struct Geom {
    uint32_t h, w, cn;
    uint32_t nc;          // components: 1 or 3
    uint32_t sub;         // 1: 4:2:0 (16 x 16 MCU: four Y blocks, Cb, Cr), 0: 8 x 8 MCU
    uint32_t bpm;         // blocks per MCU: 1, 3 or 6
    uint32_t mcux, mcuy, nmcu;
    uint32_t restart;     // MCUs per restart interval
    uint32_t nint;        // intervals
    uint32_t nblocks;
    uint32_t ibl;         // blocks of a full interval
};

__host__ __device__ inline bool make_geom(int h, int w, int cn, int subsampling, int restart_mcus, Geom& g)
{
    if ((cn != 1 && cn != 3 && cn != 4) || (subsampling != kSub444 && subsampling != kSub420) || h < 1 || w < 1 || h > 65535 || w > 65535 ||
        restart_mcus < 1 || restart_mcus > 65535)
        return false;
    g.h = (uint32_t)h, g.w = (uint32_t)w, g.cn = (uint32_t)cn;
    g.nc = cn == 1 ? 1u : 3u;
    g.sub = (g.nc == 3 && subsampling == kSub420) ? 1u : 0u;
    const uint32_t m = g.sub ? 16u : 8u;
    g.bpm = g.nc == 1 ? 1u : (g.sub ? 6u : 3u);
    g.mcux = (g.w + m - 1) / m, g.mcuy = (g.h + m - 1) / m;
    g.nmcu = g.mcux * g.mcuy;
    g.restart = (uint32_t)restart_mcus;
    g.nint = (g.nmcu + g.restart - 1) / g.restart;
    g.nblocks = g.nmcu * g.bpm;  // at most 8192 * 8192 * 3
    g.ibl = g.restart * g.bpm;
    return true;
}

// bytes of the intervals before stuffing and markers: every block at its longest, one pad byte per interval (a multiple of kPiece)
__host__ __device__ inline uint64_t raw_bound(const Geom& g)
{
    const uint64_t n = (uint64_t)g.nblocks * kMaxBlockBytes + g.nint;
    return (n + kPiece - 1) / kPiece * kPiece;
}

// bytes the scan can need: every byte stuffed, one marker per interval
__host__ __device__ inline uint64_t scan_bound(const Geom& g)
{
    return 2 * ((uint64_t)g.nblocks * kMaxBlockBytes + g.nint) + 2 * (uint64_t)g.nint;
}

// where block b of the scan lies: its component, and its first sample in the component's plane
struct BlockPos {
    uint32_t comp, x0, y0;
};

__host__ __device__ inline BlockPos block_pos(const Geom& g, uint32_t b)
{
    const uint32_t mcu = b / g.bpm, k = b - mcu * g.bpm;
    const uint32_t my = mcu / g.mcux, mx = mcu - my * g.mcux;
    BlockPos p;
    if (g.sub && k < 4) {
        p.comp = 0, p.x0 = mx * 16 + (k & 1u) * 8, p.y0 = my * 16 + (k >> 1) * 8;
    } else {
        p.comp = g.sub ? k - 3 : k, p.x0 = mx * 8, p.y0 = my * 8;
    }
    return p;
}

// the block whose DC the difference of block b is taken against, or b itself where the prediction is 0 (an interval's first block
// of each component)
__host__ __device__ inline uint32_t dc_predecessor(const Geom& g, uint32_t b)
{
    const uint32_t mcu = b / g.bpm, k = b - mcu * g.bpm;
    if (g.sub && k >= 1 && k < 4)
        return b - 1;
    if (mcu % g.restart == 0)
        return b;
    return (g.sub && k == 0) ? b - 3 : b - g.bpm;
}

// JFIF full-range BT.601 in 16-bit fixed point, of one pixel in cv2 channel order (B, G, R[, A])
__host__ __device__ inline int ycc(const uint8_t* px, uint32_t comp)
{
    const int b = px[0], g = px[1], r = px[2];
    if (comp == 0)
        return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    if (comp == 1)
        return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
    return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

// sample (x, y) of a component's plane, before the level shift.  The image is padded by repeating its last column and row, then 4:2:0
// chroma is the mean of the 2 x 2 cell, rounded half up.
__host__ __device__ inline int plane_sample(const uint8_t* img, int64_t pitch, const Geom& g, uint32_t comp, uint32_t x, uint32_t y)
{
    if (g.nc == 1) {
        const uint32_t xx = x < g.w ? x : g.w - 1, yy = y < g.h ? y : g.h - 1;
        return img[(int64_t)yy * pitch + (int64_t)xx * g.cn];
    }
    if (!(g.sub && comp)) {
        const uint32_t xx = x < g.w ? x : g.w - 1, yy = y < g.h ? y : g.h - 1;
        return ycc(img + (int64_t)yy * pitch + (int64_t)xx * g.cn, comp);
    }
    const uint32_t xa = 2 * x < g.w ? 2 * x : g.w - 1, xb = 2 * x + 1 < g.w ? 2 * x + 1 : g.w - 1;
    const uint32_t ya = 2 * y < g.h ? 2 * y : g.h - 1, yb = 2 * y + 1 < g.h ? 2 * y + 1 : g.h - 1;
    const uint8_t *ra = img + (int64_t)ya * pitch, *rb = img + (int64_t)yb * pitch;
    return (ycc(ra + (int64_t)xa * g.cn, comp) + ycc(ra + (int64_t)xb * g.cn, comp) + ycc(rb + (int64_t)xa * g.cn, comp) +
            ycc(rb + (int64_t)xb * g.cn, comp) + 2) >> 2;
}

__host__ __device__ inline int descale(int x, int n)
{
    return (x + (1 << (n - 1))) >> n;
}

// One pass of the IJG "islow" forward DCT over eight values, in place: 13-bit constants.  The first pass leaves two extra bits, the
// second removes them; the whole transform is scaled by 8.
template <bool FIRST>
__host__ __device__ inline void fdct_pass(int d[8])
{
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    constexpr int n = FIRST ? 11 : 15;
    d[0] = FIRST ? (t10 + t11) * 4 : descale(t10 + t11, 2);
    d[4] = FIRST ? (t10 - t11) * 4 : descale(t10 - t11, 2);
    int z1 = (t12 + t13) * 4433;
    d[2] = descale(z1 + t13 * 6270, n);
    d[6] = descale(z1 - t12 * 15137, n);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int m4 = t4 * 2446, m5 = t5 * 16819, m6 = t6 * 25172, m7 = t7 * 12299;
    z1 *= -7373, z2 *= -20995;
    z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
    d[7] = descale(m4 + z1 + z3, n);
    d[5] = descale(m5 + z2 + z4, n);
    d[3] = descale(m6 + z2 + z3, n);
    d[1] = descale(m7 + z1 + z4, n);
}

// the DCT output (scaled by 8) divided by 8 * q, rounded half away from zero
__host__ __device__ inline int quantise(int v, int q)
{
    const uint32_t a = (uint32_t)(v < 0 ? -v : v), c = (a + 4u * (uint32_t)q) / (8u * (uint32_t)q);
    return v < 0 ? -(int)c : (int)c;
}

// zigzag position of a row-major index
__host__ __device__ inline int zigzag_of(int natural)
{
    // the position on its anti-diagonal, walked upwards on even diagonals and downwards on odd ones
    const int r = natural >> 3, c = natural & 7, s = r + c;
    const int before = s < 8 ? s * (s + 1) / 2 : 64 - (15 - s) * (16 - s) / 2;
    const int lo = s < 8 ? 0 : s - 7;  // the smallest row (and column) on the diagonal
    return before + ((s & 1) ? r - lo : c - lo);
}

__host__ __device__ inline int bit_length(uint32_t a)
{
    return a ? 32 - __builtin_clz(a) : 0;
}

// Code tables: one entry per symbol, (length << 16) | code.  tab.dc[t][category], tab.ac[t][run << 4 | size], t = 0 luminance,
// 1 chrominance; q[t][row-major index].
struct Tables {
    uint16_t q[2][64];
    uint32_t dc[2][16];
    uint32_t ac[2][256];
};

// The entropy coder of one block: zz = 64 coefficients in zigzag order, pred = the DC it is predicted from.  Calls
// emit(bits, length) for every token in order, bits < 2^length, length <= 26: the DC difference's code with its amplitude, every
// ZRL, every non-zero AC coefficient's run / size code with its amplitude, and EOB where the last coefficient is zero.
template <class ZZ, class Emit>
__host__ __device__ inline void encode_block(const ZZ& zz, int pred, const uint32_t* dc, const uint32_t* ac, Emit&& emit)
{
    const int d = (int)zz(0) - pred;
    int s = bit_length((uint32_t)(d < 0 ? -d : d));
    uint32_t e = dc[s];
    emit(((e & 0xffffu) << s) | ((uint32_t)(d < 0 ? d - 1 : d) & ((1u << s) - 1u)), (int)(e >> 16) + s);
    int run = 0;
    for (int k = 1; k < 64; k++) {
        const int v = (int)zz(k);
        if (v == 0) {
            run++;
            continue;
        }
        for (; run > 15; run -= 16)
            emit(ac[0xf0] & 0xffffu, (int)(ac[0xf0] >> 16));
        s = bit_length((uint32_t)(v < 0 ? -v : v));
        e = ac[(run << 4) | s];
        emit(((e & 0xffffu) << s) | ((uint32_t)(v < 0 ? v - 1 : v) & ((1u << s) - 1u)), (int)(e >> 16) + s);
        run = 0;
    }
    if (run)
        emit(ac[0] & 0xffffu, (int)(ac[0] >> 16));
}

// The symbols encode_block codes for a block, for the optimised tables (jpeg_opt_core.hpp): the same walk over a table whose entry of
// symbol i is the 16-bit code i (identity_entry), so that every token carries its symbol in front of its amplitude.  Calls
// count(is_dc, symbol) once per token: the DC category, every ZRL (0xF0), every run / size symbol, and EOB (0) where encode_block emits it.
__host__ __device__ inline uint32_t identity_entry(int symbol)
{
    return (16u << 16) | (uint32_t)symbol;
}

template <class ZZ, class Count>
__host__ __device__ inline void block_symbols(const ZZ& zz, int pred, const uint32_t* identity, Count&& count)
{
    bool dc = true;
    encode_block(zz, pred, identity, identity, [&](uint32_t bits, int len) {
        count(dc, (int)(bits >> (len - 16)));
        dc = false;
    });
}

}  // namespace jpeg
}  // namespace v1c
