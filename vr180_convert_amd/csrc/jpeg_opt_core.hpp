// jpeg_opt_core.hpp -- the optimised Huffman tables of the device JPEG encoder (optimize=True: kernels_jpeg_opt.hip, jpeg.hip): the
// symbol histograms of an image, and the table a histogram gives -- libjpeg's jpeg_gen_optimal_table as INTEGRATION.md section 7
// states it.  __host__ __device__ over a `Wave` that says how many lanes run the procedure together and how they agree on a minimum,
// so that tests/host_jpeg_opt/jpeg_opt_emul.hip runs exactly this code with one lane against the plain-Python restatement
// (tests/jpg_opt_ref.py).  Integer arithmetic throughout: the tables are a pure function of the counts.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jpeg_core.hpp"

namespace v1c {
namespace jpeg {

// The four tables in the order of the DHT segment: DC luminance, AC luminance, DC chrominance, AC chrominance (Tc << 4 | Th = 0x00,
// 0x10, 0x01, 0x11).  Table t is Tables::dc[t >> 1] (t even, 16 entries) or Tables::ac[t >> 1] (t odd, 256 entries).
constexpr int kOptTables = 4;
constexpr int kReserved = 256;     // the symbol of frequency 1 that keeps the all-ones code out of the table
// The longest code before the limit to 16 bits.  A code of n bits needs a total count of at least the n-th Fibonacci number; the AC
// symbols of a 65535 x 65535 image in 4:4:4 are fewer than 2^40 < F(60), so no code passes 59 bits.
constexpr int kMaxCodeSize = 64;
constexpr int kDhtTableMax = 16 + 256;  // BITS and HUFFVAL of one table

// A DC table has at most 12 symbols and the reserved one: 13 leaves, so no code passes 12 bits, the limit to 16 never acts on it and
// the longest DC token is 12 + 11 = 23 bits, inside encode_block's 26.  An AC token is at most 16 + 10 = 26 bits as with the Annex K
// tables.  So a block is at most 23 + 63 * 26 = 1661 bits: within the kMaxBlockBytes every region of the workspace and
// v1c_jpeg_bound are sized by.  The packer of jpeg_kernels.hpp holds fewer than 32 bits between tokens: 31 + 26 < 64.
static_assert(12 + 11 + 63 * 26 <= 8 * kMaxBlockBytes, "an optimised block must fit the bytes every region is sized by");

struct Hist {
    uint64_t n[kOptTables][256];  // 64-bit: a 65535 x 65535 image has more than 2^32 AC symbols
};

// What the host needs of an image's tables for the DHT segment: per table the bytes of BITS and HUFFVAL, and their number (0: not built)
struct DhtRecord {
    uint32_t len[kOptTables];
    uint8_t body[kOptTables][kDhtTableMax];
};

struct BuildScratch {
    uint64_t freq[257];
    uint16_t size[257];   // code size so far
    uint16_t root[257];   // the entry that carries the frequency of the symbol's subtree
    uint32_t bits[kMaxCodeSize + 1];
};

// An entry as one word for the search of a step: the frequency above the index counted down, so that the smallest key is the entry of
// the smallest frequency and, among equals, of the LARGEST index (libjpeg's ascending scans with `<=`).  A frequency is at most the
// image's symbols of a kind, fewer than 2^40 (above): it fits the 55 bits.
constexpr uint64_t kNoEntry = ~0ull;

__host__ __device__ inline uint64_t entry_key(uint64_t freq, int index)
{
    return (freq << 9) | (uint64_t)(kReserved - index);
}

__host__ __device__ inline int entry_of(uint64_t key)
{
    return key == kNoEntry ? -1 : kReserved - (int)(key & 511u);
}

// the builder on one lane (the host emulation)
struct OneLane {
    __host__ __device__ int lane() const { return 0; }
    __host__ __device__ int lanes() const { return 1; }
    __host__ __device__ void barrier() const {}
    __host__ __device__ void least_two(uint64_t&, uint64_t&) const {}
};

// One step's search: c1, the non-zero entry of the smallest frequency, and c2, the smallest among the others; -1 where there is none.
// Every lane keeps the two smallest keys of its entries, then the lanes agree (Wave::least_two: the two smallest of all lanes' keys).
template <class Wave>
__host__ __device__ inline void least_entries(const uint64_t* freq, const Wave& wv, int& c1, int& c2)
{
    uint64_t k1 = kNoEntry, k2 = kNoEntry;
    for (int i = wv.lane(); i <= kReserved; i += wv.lanes()) {
        const uint64_t f = freq[i];
        if (!f)
            continue;
        const uint64_t k = entry_key(f, i);
        if (k < k1)
            k2 = k1, k1 = k;
        else if (k < k2)
            k2 = k;
    }
    wv.least_two(k1, k2);
    c1 = entry_of(k1), c2 = entry_of(k2);
}

// The table of one histogram.  hist: nsym counts (16 or 256); codes: the nsym entries (length << 16) | code of the Tables, 0 for a
// symbol that does not occur; body / body_len: BITS, then HUFFVAL, and their number of bytes.  All lanes of `wv` call it together.
template <class Wave>
__host__ __device__ inline void build_table(const uint64_t* hist, int nsym, BuildScratch& s, uint32_t* codes, uint8_t* body, uint32_t* body_len,
                                            const Wave& wv)
{
    const int lane = wv.lane(), nl = wv.lanes();
    for (int i = lane; i <= kReserved; i += nl) {
        s.freq[i] = i < nsym ? hist[i] : (i == kReserved ? 1u : 0u);
        s.size[i] = 0;
        s.root[i] = (uint16_t)i;
    }
    for (int i = lane; i <= kMaxCodeSize; i += nl)
        s.bits[i] = 0;
    for (int i = lane; i < nsym; i += nl)
        codes[i] = 0;
    wv.barrier();
    // the two least frequent entries become one, every symbol below either grows by a bit: until one entry is left
    for (;;) {
        int c1, c2;
        least_entries(s.freq, wv, c1, c2);
        if (c2 < 0)
            break;
        wv.barrier();
        if (lane == 0) {
            s.freq[c1] += s.freq[c2];
            s.freq[c2] = 0;
        }
        for (int i = lane; i <= kReserved; i += nl) {
            const int r = s.root[i];
            if (r == c1 || r == c2) {
                s.size[i]++;
                s.root[i] = (uint16_t)c1;
            }
        }
        wv.barrier();
    }
    if (lane == 0) {
        for (int i = 0; i <= kReserved; i++)
            if (s.size[i])
                s.bits[s.size[i] < kMaxCodeSize ? s.size[i] : kMaxCodeSize]++;
        // Annex K.2, figure K.3: a pair of the longest codes moves up beside a shorter code's new sibling, until none passes 16 bits
        for (int i = kMaxCodeSize; i > 16; i--)
            while (s.bits[i] > 0) {
                int j = i - 2;
                while (s.bits[j] == 0)
                    j--;
                s.bits[i] -= 2;
                s.bits[i - 1]++;
                s.bits[j + 1] += 2;
                s.bits[j]--;
            }
        int i = 16;
        while (s.bits[i] == 0)
            i--;
        s.bits[i]--;  // the reserved symbol's code point
        uint32_t n = 0;
        for (i = 1; i <= 16; i++) {
            body[i - 1] = (uint8_t)s.bits[i];
            n += s.bits[i];
        }
        *body_len = 16 + n;
    }
    // HUFFVAL: the symbols by code size, then by value: every symbol's place is the number of symbols in front of it
    for (int j = lane; j < 256; j += nl) {
        const int sj = s.size[j];
        if (!sj)
            continue;
        int at = 0;
        for (int k = 0; k < 256; k++) {
            const int sk = s.size[k];
            at += (sk && (sk < sj || (sk == sj && k < j))) ? 1 : 0;
        }
        body[16 + at] = (uint8_t)j;
    }
    wv.barrier();
    // canonical codes (Annex C) in that order
    if (lane == 0) {
        uint32_t code = 0;
        int p = 0;
        for (int n = 1; n <= 16; n++) {
            for (uint32_t i = 0; i < s.bits[n]; i++)
                codes[body[16 + p++]] = ((uint32_t)n << 16) | code++;
            code <<= 1;
        }
    }
    wv.barrier();
}

// the histogram a block's symbols go to: t = 0 luminance, 1 chrominance
__host__ __device__ inline int hist_of(bool dc, int t)
{
    return 2 * t + (dc ? 0 : 1);
}

// the DHT segment's body from an image's record: per built table Tc << 4 | Th, BITS, HUFFVAL.  out: 4 * (1 + kDhtTableMax) bytes
inline uint32_t dht_body(const DhtRecord& r, uint8_t* out)
{
    const uint8_t ids[kOptTables] = {0x00, 0x10, 0x01, 0x11};
    uint32_t n = 0;
    for (int t = 0; t < kOptTables; t++) {
        if (!r.len[t])
            continue;
        out[n++] = ids[t];
        for (uint32_t i = 0; i < r.len[t]; i++)
            out[n++] = r.body[t][i];
    }
    return n;
}

}  // namespace jpeg
}  // namespace v1c
