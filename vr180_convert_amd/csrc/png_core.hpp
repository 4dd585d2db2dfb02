// png_core.hpp -- per-byte and per-segment arithmetic of the device PNG encoder (kernels_png.hip, png.hip).
//
// __host__ __device__ so that tests/host_png/png_emul.hip runs exactly this code on the host against the NumPy restatement
// (tests/png_ref.py).  Integer arithmetic throughout: the stream is a pure function of the pixels and the parameters
// (INTEGRATION.md section 6).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace v1c {
namespace png {

constexpr int kSeg = 256;        // scanline bytes of a band per segment: runs never cross a multiple of it (counted from the band's start)
constexpr int kMinMatch = 4;     // a run of fewer equal bytes (after the byte they repeat) stays literals
constexpr int kSymbols = 286;    // literal / length alphabet
constexpr int kEob = 256;
constexpr int kMaxBits = 15;
constexpr uint32_t kAdlerBase = 65521;
constexpr uint32_t kStoredMax = 65535;  // bytes per stored block
constexpr int kFilterUp = 2, kFilterPaeth = 4;

constexpr int kHistStride = 288;    // counters per band (286 used)
constexpr int kSegsPerGroup = 64;   // segments one workgroup of four waves walks: 16 KB of scanlines

// what pass 2 needs to know of a band (written by the host between the passes)
struct BandDev {
    uint64_t token_bit0;  // bit of the stream at which the band's first token starts (8 * offset + header bits)
    uint64_t byte0;       // the band's first byte of the stream
    uint32_t stored;
    uint32_t pad;
};

// a word the host asks the device to OR into the stream
struct OrWord {
    uint64_t word;   // index of the 32-bit word of the stream
    uint32_t value;
    uint32_t pad;
};

enum TokenKind { kNone = 0, kLiteral = 1, kMatch = 2 };

// one raw scanline byte of row `row`, `x` bytes into the row's samples (PNG order: gray / RGB / RGBA, 16-bit big-endian) read from a
// cv2-ordered image (gray / BGR / BGRA, native little-endian samples).  bpp = bytes per pixel: 1, 3, 4 (8-bit) or 2, 6, 8 (16-bit).
__host__ __device__ inline uint32_t raw_byte(const uint8_t* img, int64_t pitch, int bpp, uint32_t row, uint32_t x)
{
    const int nb = (bpp == 2 || bpp >= 6) ? 2 : 1;
    const int cn = bpp / nb;
    const uint32_t px = x / (uint32_t)bpp, wi = x - px * (uint32_t)bpp;
    const uint32_t c = nb == 2 ? wi >> 1 : wi, bi = nb == 2 ? wi & 1u : 0u;
    const uint32_t sc = (cn >= 3 && c < 3) ? 2 - c : c;
    const uint32_t off = sc * (uint32_t)nb + (nb == 2 ? 1u - bi : 0u);
    return img[(int64_t)row * pitch + (int64_t)px * bpp + off];
}

__host__ __device__ inline uint32_t paeth(int a, int b, int c)
{
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    return (uint32_t)((pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c));
}

// byte `col` of filtered scanline `row` (col 0 is the filter type).  Both filters predict from UNFILTERED neighbours; the row above
// row 0 and the pixel left of column 0 are zero.
__host__ __device__ inline uint32_t filtered_byte(const uint8_t* img, int64_t pitch, int bpp, int filter, uint32_t row, uint32_t col)
{
    if (col == 0)
        return (uint32_t)filter;
    const uint32_t x = col - 1;
    const uint32_t cur = raw_byte(img, pitch, bpp, row, x);
    const uint32_t up = row ? raw_byte(img, pitch, bpp, row - 1, x) : 0u;
    if (filter == kFilterUp)
        return (cur - up) & 255u;
    const bool has_left = x >= (uint32_t)bpp;
    const uint32_t left = has_left ? raw_byte(img, pitch, bpp, row, x - bpp) : 0u;
    const uint32_t ul = (has_left && row) ? raw_byte(img, pitch, bpp, row - 1, x - bpp) : 0u;
    return (cur - paeth((int)left, (int)up, (int)ul)) & 255u;
}

__host__ __device__ inline int ctz64(uint64_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __ffsll((unsigned long long)v) - 1;
#else
    return __builtin_ctzll(v);
#endif
}

// eq[4]: bit p of the 256-bit mask says that byte p of the segment equals byte p - 1 (bit 0 is always clear).  The number of set bits
// from position 64 * c + b upwards, without a gap.
__host__ __device__ inline int run_up(const uint64_t eq[4], int c, int b)
{
    int n = 0;
    bool open = true;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        if (w < c)
            continue;
        const int s = w == c ? b : 0;
        const uint64_t x = ~(eq[w] >> s);  // (the zeros shifted in at the top end the count at the word's edge)
        const int avail = 64 - s;
        int k = x ? ctz64(x) : 64;
        k = k < avail ? k : avail;
        n += open ? k : 0;
        open = open && k == avail;
    }
    return n;
}

// The tokenisation rule.  Inside a segment, a maximal run of L >= 1 bytes that equal the byte before them becomes one match of
// distance 1 and length L if L >= kMinMatch, and L literals otherwise; every other byte is a literal.  (L <= kSeg - 1 < 258: a
// match is never split.)  This is what a greedy left-to-right scan that takes the longest distance-1 match of at least kMinMatch
// gives.  Returns the kind of token that STARTS at byte 64 * c + b and, for a match, its length.
__host__ __device__ inline int classify(const uint64_t eq[4], int c, int b, int* length)
{
    *length = 0;
    if (!((eq[c] >> b) & 1))
        return kLiteral;
    // the three mask bits below this position: bit 2 is position - 1
    const uint64_t prev = c ? eq[c > 0 ? c - 1 : 0] >> 61 : 0;  // (the top three bits of the word below)
    const uint64_t same = eq[c] >> (b >= 3 ? b - 3 : 0), edge = (eq[c] << (b < 3 ? 3 - b : 0)) | (prev >> (b < 3 ? b : 0));
    const uint32_t lo3 = (uint32_t)((b >= 3 ? same : edge) & 7u);
    const int below = (lo3 & 4u) ? ((lo3 & 2u) ? ((lo3 & 1u) ? 3 : 2) : 1) : 0;
    const int up = run_up(eq, c, b);
    if (below + up < kMinMatch)
        return kLiteral;
    if (below)
        return kNone;
    *length = up;
    return kMatch;
}

// deflate's length alphabet (RFC 1951 3.2.5): symbol, number of extra bits and their value for a match length 3..258
__host__ __device__ inline void length_symbol(int length, int* sym, int* xbits, int* xval)
{
    const int l = length - 3;
    if (length == 258) {
        *sym = 285, *xbits = 0, *xval = 0;
    } else if (l < 8) {
        *sym = 257 + l, *xbits = 0, *xval = 0;
    } else {
        const int k = 29 - __builtin_clz((unsigned)l);  // floor(log2 l) - 2
        *sym = 261 + 4 * k + ((l >> k) & 3), *xbits = k, *xval = l & ((1 << k) - 1);
    }
}

// A band's code table has one entry per symbol: (bit-reversed code << 4) | length, so that a code goes out LSB first.
// The bits of one token and their number: a literal is its code; a match is the length code, the extra bits and the single
// distance code (one zero bit).
__host__ __device__ inline uint32_t token_bits(const uint32_t* table, int kind, uint32_t byte, int length, int* nbits)
{
    if (kind == kNone) {
        *nbits = 0;
        return 0;
    }
    if (kind == kLiteral) {
        const uint32_t e = table[byte];
        *nbits = (int)(e & 15u);
        return e >> 4;
    }
    int sym, xb, xv;
    length_symbol(length, &sym, &xb, &xv);
    const uint32_t e = table[sym];
    const int cl = (int)(e & 15u);
    *nbits = cl + xb + 1;
    return (e >> 4) | ((uint32_t)xv << cl);
}

__host__ __device__ inline int token_symbol(int kind, uint32_t byte, int length)
{
    if (kind == kLiteral)
        return (int)byte;
    int sym, xb, xv;
    length_symbol(length, &sym, &xb, &xv);
    return sym;
}

// where byte i of a band's scanlines lies inside the band's stored-block form (5 header bytes in front of every 65535 data bytes)
__host__ __device__ inline uint64_t stored_position(uint32_t i)
{
    return (uint64_t)i + 5u * (uint64_t)(i / kStoredMax + 1u);
}

__host__ __device__ inline uint64_t stored_size(uint32_t nbytes)
{
    return (uint64_t)nbytes + 5u * (uint64_t)((nbytes + kStoredMax - 1u) / kStoredMax);
}

}  // namespace png
}  // namespace v1c
