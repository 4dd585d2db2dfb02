// jpeg_host.hpp -- host side of the device JPEG encoder: the Annex K tables of ISO/IEC 10918-1, the quantisation tables of a quality,
// the code tables the kernels read, the header segments of the file, and the rule of a DHT body that a caller hands back.  Shared by
// jpeg.hip, the lossless entries and tests/host_jpeg/jpeg_emul.hip.
#pragma once

#include <cstring>
#include <vector>

#include "jpeg_core.hpp"

namespace v1c {
namespace jpeg {

// Annex K.1 / K.2, row-major
constexpr uint8_t kQLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                                69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55, 64,
                                81, 104, 113, 92, 49, 64,  78,  87,  103, 121, 120, 101, 72, 92,  95,  98,  112, 100, 103, 99};
constexpr uint8_t kQChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                  99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                  99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// Annex K.3 - K.6: the number of codes of each length 1 ... 16, then the symbols in code order
struct HuffSpec {
    uint8_t bits[16];
    int n;
    uint8_t vals[162];
};

constexpr HuffSpec kDcLuma = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr HuffSpec kDcChroma = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, 12, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}};
constexpr HuffSpec kAcLuma = {
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
    162,
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
     0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
     0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
     0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
     0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
     0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
     0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa}};
constexpr HuffSpec kAcChroma = {
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
    162,
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
     0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
     0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
     0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
     0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
     0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
     0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
     0xfa}};

// the IJG quality rule
inline int quant_entry(int base, int quality)
{
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    const int v = (base * s + 50) / 100;
    return v < 1 ? 1 : (v > 255 ? 255 : v);
}

// canonical codes (Annex C) by symbol
inline void code_table(const HuffSpec& spec, uint32_t* out, int size)
{
    std::memset(out, 0, (size_t)size * 4);
    uint32_t code = 0;
    int k = 0;
    for (int n = 1; n <= 16; n++) {
        for (int i = 0; i < spec.bits[n - 1]; i++)
            out[spec.vals[k++]] = ((uint32_t)n << 16) | code++;
        code <<= 1;
    }
}

inline void make_tables(int quality, Tables& t)
{
    for (int i = 0; i < 64; i++) {
        t.q[0][i] = (uint16_t)quant_entry(kQLuma[i], quality);
        t.q[1][i] = (uint16_t)quant_entry(kQChroma[i], quality);
    }
    code_table(kDcLuma, t.dc[0], 16);
    code_table(kDcChroma, t.dc[1], 16);
    code_table(kAcLuma, t.ac[0], 256);
    code_table(kAcChroma, t.ac[1], 256);
}

// whether a DHT body is whole tables in the segment's order: the two of one component, or the four of three
inline bool whole_tables(const uint8_t* dht, uint32_t dht_size, uint32_t nc)
{
    const uint8_t ids[4] = {0x00, 0x10, 0x01, 0x11};
    uint32_t at = 0, tables = 0;
    while (at < dht_size && tables < 4) {
        if (dht[at] != ids[tables] || at + 17 > dht_size)
            return false;
        uint32_t nsym = 0;
        for (int i = 0; i < 16; i++)
            nsym += dht[at + 1 + i];
        if (nsym < 1 || nsym > 256)
            return false;
        at += 17 + nsym, tables++;
    }
    return at == dht_size && tables == (nc == 1 ? 2u : 4u);
}

inline void put_segment(std::vector<uint8_t>& out, int marker, const std::vector<uint8_t>& body)
{
    const size_t n = body.size() + 2;
    out.insert(out.end(), {0xff, (uint8_t)marker, (uint8_t)(n >> 8), (uint8_t)n});
    out.insert(out.end(), body.begin(), body.end());
}

// SOI, APP0 (JFIF 1.01, aspect 1:1), DQT, SOF0, DHT, DRI, SOS: everything in front of the scan.  dht: the DHT segment's body of an
// optimising encode (jpeg_opt_core.hpp), or NULL for the Annex K tables
inline std::vector<uint8_t> file_header(const Geom& g, int quality, const uint8_t* dht = nullptr, uint32_t dht_size = 0)
{
    Tables t;
    make_tables(quality, t);
    std::vector<uint8_t> out = {0xff, 0xd8};
    put_segment(out, 0xe0, {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
    std::vector<uint8_t> b;
    for (uint32_t i = 0; i < (g.nc == 1 ? 1u : 2u); i++) {
        b.push_back((uint8_t)i);
        const size_t at = b.size();
        b.resize(at + 64);
        for (int n = 0; n < 64; n++)
            b[at + zigzag_of(n)] = (uint8_t)t.q[i][n];
    }
    put_segment(out, 0xdb, b);
    b = {8, (uint8_t)(g.h >> 8), (uint8_t)g.h, (uint8_t)(g.w >> 8), (uint8_t)g.w, (uint8_t)g.nc};
    for (uint32_t i = 0; i < g.nc; i++)
        b.insert(b.end(), {(uint8_t)(i + 1), (uint8_t)((i == 0 && g.sub) ? 0x22 : 0x11), (uint8_t)(i ? 1 : 0)});
    put_segment(out, 0xc0, b);
    b.clear();
    const HuffSpec* specs[4] = {&kDcLuma, &kAcLuma, &kDcChroma, &kAcChroma};
    const uint8_t ids[4] = {0x00, 0x10, 0x01, 0x11};
    for (uint32_t i = 0; i < (g.nc == 1 ? 2u : 4u) && !dht; i++) {
        b.push_back(ids[i]);
        b.insert(b.end(), specs[i]->bits, specs[i]->bits + 16);
        b.insert(b.end(), specs[i]->vals, specs[i]->vals + specs[i]->n);
    }
    if (dht)
        b.assign(dht, dht + dht_size);
    put_segment(out, 0xc4, b);
    put_segment(out, 0xdd, {(uint8_t)(g.restart >> 8), (uint8_t)g.restart});
    b = {(uint8_t)g.nc};
    for (uint32_t i = 0; i < g.nc; i++)
        b.insert(b.end(), {(uint8_t)(i + 1), (uint8_t)(i ? 0x11 : 0x00)});
    b.insert(b.end(), {0, 63, 0});
    put_segment(out, 0xda, b);
    return out;
}

}  // namespace jpeg
}  // namespace v1c
