// jpegdec_core.hpp -- per-symbol, per-block and per-pixel arithmetic of the device JPEG decoder (kernels_jpegdec.hip, jpegdec.hip): the
// geometry, the bit reader, the step of the Huffman decoder over one symbol, F_i over one subsequence, the passes of libjpeg's accurate
// integer inverse DCT, its triangle-filter chroma upsampling and its 16-bit YCbCr conversion.
//
// __host__ __device__ so that tests/host_jpegdec/jpegdec_emul.hip runs exactly this code on the host against the restatement
// (tests/jpgdec_ref.py).  Integer arithmetic throughout: the pixels are a pure function of the file.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace v1c {
namespace jpegdec {

constexpr int kPiece = 16;               // bytes of the stuffed scan one lane of the unstuffing kernels takes
constexpr uint32_t kDefaultSubseqBits = 1024;
constexpr int kLutBits = 8;              // codes up to this length are found by one lookup

struct Geom {
    uint32_t h, w, nc;
    uint32_t hs, vs;                     // luma sampling factors (chroma: 1 x 1)
    uint32_t ny, bpm;                    // luma blocks and all blocks of an MCU
    uint32_t mcux, mcuy, nmcu, nblocks;
    uint32_t interval;                   // MCUs of a full segment (the restart interval, or all MCUs)
    uint32_t nseg, ibl;                  // segments; blocks of a full segment
    uint32_t cw, ch;                     // chroma samples the frame covers: ceil(w / hs), ceil(h / vs)
    uint8_t tq[3], td[3], ta[3], pad[3]; // per component: quantisation, DC and AC table
};

__host__ __device__ inline void finish_geom(Geom& g)
{
    g.ny = g.hs * g.vs;
    g.bpm = g.ny + (g.nc == 3 ? 2u : 0u);
    g.mcux = (g.w + 8 * g.hs - 1) / (8 * g.hs), g.mcuy = (g.h + 8 * g.vs - 1) / (8 * g.vs);
    g.nmcu = g.mcux * g.mcuy;
    g.nblocks = g.nmcu * g.bpm;
    g.cw = (g.w + g.hs - 1) / g.hs, g.ch = (g.h + g.vs - 1) / g.vs;
}

// component of block k of an MCU
__host__ __device__ inline uint32_t comp_of(const Geom& g, uint32_t k)
{
    return k < g.ny ? 0u : k - g.ny + 1;
}

// One Huffman table as the decoder reads it: codes of up to kLutBits bits by one lookup (length << 8 | symbol, 0: a longer code or
// none), longer ones by the canonical arrays (ISO/IEC 10918-1 F.2.2.3): a code of n bits is one if it is <= maxcode[n], and its
// symbol is vals[code + valoff[n]].
struct Table {
    uint16_t lut[1 << kLutBits];
    int32_t maxcode[18];                 // -1 where no code has the length; [17]: unused
    int32_t valoff[18];
    uint8_t vals[256];
};

struct Tables {
    uint16_t q[4][64];                   // row-major
    Table dc[4], ac[4];
};

// the tables of every block of an MCU: four bits each of `dcsel` / `acsel` index `dc` / `ac`
struct TablePair {
    const Table *dcs, *acs;
    uint32_t dcsel, acsel;
    __host__ __device__ const Table& dc(uint32_t c) const { return dcs[(dcsel >> (4 * c)) & 3u]; }
    __host__ __device__ const Table& ac(uint32_t c) const { return acs[(acsel >> (4 * c)) & 3u]; }
};

// 32 bits of the unstuffed stream from bit p on, most significant first.  `u` holds whole words, two of them behind the last byte.
__host__ __device__ inline uint32_t peek32(const uint32_t* u, uint32_t p)
{
    const uint32_t hi = __builtin_bswap32(u[p >> 5]), lo = __builtin_bswap32(u[(p >> 5) + 1]);
    const uint32_t s = p & 31u;
    return s ? (hi << s) | (lo >> (32u - s)) : hi;
}

// the code at the head of w: length << 8 | symbol, 0 where the bits start no code.  The loop over the lengths is bounded by 16.
__host__ __device__ inline uint32_t find_code(const Table& t, uint32_t w)
{
    const uint32_t e = t.lut[w >> (32 - kLutBits)];
    if (e)
        return e;
    for (int n = kLutBits + 1; n <= 16; n++) {
        const int32_t code = (int32_t)(w >> (32 - n));
        if (code <= t.maxcode[n])
            return (uint32_t)n << 8 | t.vals[(code + t.valoff[n]) & 255];  // (in range for the tables make_table accepts)
    }
    return 0;
}

struct State {
    uint32_t p;                          // bit of the next symbol in the unstuffed stream
    uint32_t zc;                         // z | c << 8: zigzag index of the next coefficient, block within the MCU
};

__host__ __device__ inline bool operator==(const State& a, const State& b)
{
    return a.p == b.p && a.zc == b.zc;
}

// The symbols that start in [s.p, end) of a segment that ends at bit E; s becomes the exit state.  Returns the blocks completed.
// The rules that make speculative decoding deterministic: bits that start no code consume one bit, a run past index 63 ends the
// block, a symbol that would pass E stops the decode at E.
// WRITE: the last pass -- coefficient k of block b goes to coef[b * 64 + k] while b < bq (decoding stops there), and the bit of the first
// invalid code, run past 63 or symbol past E is returned through *err (untouched otherwise).
template <bool WRITE>
__host__ __device__ inline uint32_t decode_span(const uint32_t* u, const TablePair& tp, uint32_t bpm, State& s, uint32_t end, uint32_t E,
                                                int16_t* coef, uint32_t b, uint32_t bq, uint32_t* err)
{
    uint32_t p = s.p, z = s.zc & 255u, c = s.zc >> 8, n = 0;
    // (every turn consumes a bit at least: the loop is bounded by the subsequence's bits)
    while (p < end && (!WRITE || b < bq)) {
        const uint32_t w = peek32(u, p);
        const uint32_t e = find_code(z == 0 ? tp.dc(c) : tp.ac(c), w);
        if (e == 0) {
            if (WRITE) {
                *err = p;
                break;
            }
            p++;
            continue;
        }
        const uint32_t len = e >> 8, sym = e & 255u;
        const uint32_t sz = z == 0 ? sym : sym & 15u, run = z == 0 ? 0u : sym >> 4;
        if (p + len + sz > E) {
            if (WRITE)
                *err = p;
            p = E;
            break;
        }
        int v = 0;
        if (sz) {
            v = (int)((w << len) >> (32u - sz));
            if (v < (1 << (sz - 1)))
                v -= (1 << sz) - 1;
        }
        const uint32_t p0 = p;
        p += len + sz;
        if (z == 0) {
            if (WRITE)
                coef[(size_t)b * 64] = (int16_t)v;
            z = 1;
            continue;
        }
        if (sz == 0 && run != 15) {
            z = 64;  // EOB
        } else {
            z += sz ? run : 16u;
            if (z > 63) {
                if (WRITE) {
                    *err = p0;
                    break;
                }
            } else if (sz) {
                if (WRITE)
                    coef[(size_t)b * 64 + z] = (int16_t)v;
                z++;
            } else {
                continue;
            }
        }
        if (z > 63) {
            z = 0;
            c = c + 1 == bpm ? 0u : c + 1;
            n++, b++;
        }
    }
    s.p = p, s.zc = z | c << 8;
    return n;
}

// where the DC difference of block b lies in the order the DC scan runs over (all blocks of Y, then of Cb, then of Cr), and where its
// segment's first block of the same component does: the DC is the inclusive sum at the first minus the exclusive sum at the second
__host__ __device__ inline void dc_pos(const Geom& g, uint32_t b, uint32_t& pos, uint32_t& pos0)
{
    const uint32_t mcu = b / g.bpm, k = b - mcu * g.bpm, m0 = mcu / g.interval * g.interval;
    if (k < g.ny) {
        pos = mcu * g.ny + k, pos0 = m0 * g.ny;
    } else {
        const uint32_t base = g.nmcu * g.ny + (k - g.ny) * g.nmcu;
        pos = base + mcu, pos0 = base + m0;
    }
}

// component, and first sample in the component's padded plane, of block b
struct BlockPos {
    uint32_t comp, x0, y0;
};

__host__ __device__ inline BlockPos block_pos(const Geom& g, uint32_t b)
{
    const uint32_t mcu = b / g.bpm, k = b - mcu * g.bpm;
    const uint32_t my = mcu / g.mcux, mx = mcu - my * g.mcux;
    BlockPos r;
    if (k < g.ny) {
        r.comp = 0, r.x0 = (mx * g.hs + k % g.hs) * 8, r.y0 = (my * g.vs + k / g.hs) * 8;
    } else {
        r.comp = k - g.ny + 1, r.x0 = mx * 8, r.y0 = my * 8;
    }
    return r;
}

// bytes from one row of a component's padded plane to the next; rows of it
__host__ __device__ inline uint32_t plane_pitch(const Geom& g, uint32_t comp)
{
    return g.mcux * 8 * (comp ? 1u : g.hs);
}

__host__ __device__ inline uint32_t plane_rows(const Geom& g, uint32_t comp)
{
    return g.mcuy * 8 * (comp ? 1u : g.vs);
}

// a coefficient times its quantiser entry, saturated to 16 bits.  Samples of 8 bits give dequantised values within some +-1300; the
// bound only meets files that pair 16-bit table entries with large coefficients, and it keeps both passes below exact: with inputs
// of at most 2^15 the column pass stays below 2^33 inside and 2^22 at its output, the row pass below 2^40 inside
__host__ __device__ inline int dequantise(int coef, int q)
{
    const int v = coef * q;  // (|coef| < 2^15, q < 2^16)
    return v < -32768 ? -32768 : v > 32767 ? 32767 : v;
}

// One pass of libjpeg's accurate integer ("islow") inverse DCT over eight values, in place: 13-bit constants.  The column pass takes
// dequantised coefficients and leaves two extra bits (SHIFT 11), the row pass removes them and the transform's factor 8 (SHIFT 18).
// 64-bit inside (as libjpeg's JLONG on LP64): no input that `dequantise` lets through overflows.
template <int SHIFT>
__host__ __device__ inline void idct_pass(int d[8])
{
    using L = long long;
    L z1 = (L)(d[2] + d[6]) * 4433;
    L t2 = z1 - (L)d[6] * 15137, t3 = z1 + (L)d[2] * 6270;
    L t0 = (L)(d[0] + d[4]) * 8192, t1 = (L)(d[0] - d[4]) * 8192;
    const L t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    t0 = d[7], t1 = d[5], t2 = d[3], t3 = d[1];
    z1 = t0 + t3;
    L z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const L z5 = (z3 + z4) * 9633;
    t0 *= 2446, t1 *= 16819, t2 *= 25172, t3 *= 12299;
    z1 *= -7373, z2 *= -20995;
    z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
    t0 += z1 + z3, t1 += z2 + z4, t2 += z2 + z3, t3 += z1 + z4;
    constexpr L r = 1ll << (SHIFT - 1);
    d[0] = (int)((t10 + t3 + r) >> SHIFT), d[7] = (int)((t10 - t3 + r) >> SHIFT);
    d[1] = (int)((t11 + t2 + r) >> SHIFT), d[6] = (int)((t11 - t2 + r) >> SHIFT);
    d[2] = (int)((t12 + t1 + r) >> SHIFT), d[5] = (int)((t12 - t1 + r) >> SHIFT);
    d[3] = (int)((t13 + t0 + r) >> SHIFT), d[4] = (int)((t13 - t0 + r) >> SHIFT);
}

__host__ __device__ inline int clamp255(int v)
{
    return v < 0 ? 0 : v > 255 ? 255 : v;
}

// zigzag position of a row-major index
__host__ __device__ inline int zigzag_of(int natural)
{
    const int r = natural >> 3, c = natural & 7, s = r + c;
    const int before = s < 8 ? s * (s + 1) / 2 : 64 - (15 - s) * (16 - s) / 2;
    const int lo = s < 8 ? 0 : s - 7;
    return before + ((s & 1) ? r - lo : c - lo);
}

// chroma sample of pixel (x, y) from a component's padded plane: libjpeg's triangle filter ("fancy upsampling") where the plane is more
// than two samples wide -- 3/4 of the nearer sample and 1/4 of the further one in each axis, the rounding alternating with the pixel's
// parity, neighbours clamped to the samples the frame covers -- else replication
__host__ __device__ inline int chroma_sample(const uint8_t* plane, uint32_t pitch, const Geom& g, uint32_t x, uint32_t y)
{
    if (g.hs == 1)
        return plane[(size_t)y * pitch + x];
    const uint32_t xn = x >> 1, yn = g.vs == 2 ? y >> 1 : y;
    if (g.cw <= 2)
        return plane[(size_t)yn * pitch + xn];
    const uint32_t xf = (x & 1u) ? (xn + 1 < g.cw ? xn + 1 : xn) : (xn ? xn - 1 : 0u);
    const uint8_t* rn = plane + (size_t)yn * pitch;
    if (g.vs == 1)
        return (3 * rn[xn] + rn[xf] + ((x & 1u) ? 2 : 1)) >> 2;
    const uint32_t yf = (y & 1u) ? (yn + 1 < g.ch ? yn + 1 : yn) : (yn ? yn - 1 : 0u);
    const uint8_t* rf = plane + (size_t)yf * pitch;
    const int near = 3 * rn[xn] + rf[xn], far = 3 * rn[xf] + rf[xf];
    return (3 * near + far + ((x & 1u) ? 7 : 8)) >> 4;
}

// JFIF YCbCr to B, G, R in libjpeg's 16-bit fixed point
__host__ __device__ inline void ycc_to_bgr(int y, int cb, int cr, uint8_t* bgr)
{
    cb -= 128, cr -= 128;
    bgr[0] = (uint8_t)clamp255(y + ((116130 * cb + 32768) >> 16));
    bgr[1] = (uint8_t)clamp255(y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    bgr[2] = (uint8_t)clamp255(y + ((91881 * cr + 32768) >> 16));
}

// whether byte `cur` of the stuffed scan is dropped from the unstuffed stream: the 0x00 behind a 0xFF, a 0xFF fill byte, and both bytes
// of RSTm (the scan ends in front of any other marker)
__host__ __device__ inline bool dropped(uint32_t prev, uint32_t cur, uint32_t next)
{
    return (cur == 0xffu && next != 0u) | (prev == 0xffu && (cur == 0u || (cur & 0xf8u) == 0xd0u));
}

}  // namespace jpegdec
}  // namespace v1c
