// jpeg_emul.hip -- TEST HARNESS: runs the product's JPEG arithmetic (jpeg_core.hpp: geometry, colour conversion, downsampling, DCT,
// quantisation, the entropy coder of a block) and its host side (jpeg_host.hpp: tables and header segments) on the CPU, block by
// block, in the order of the kernels' passes.
//
// Built by tests/test_jpeg_device_host.py itself (hipcc --cuda-host-only -O2 -shared -fPIC, into a temporary directory) and compared
// there with the NumPy restatement of the contract (tests/jpg_ref.py).  Not part of the product: nothing in vr180_convert_amd/ loads it.
#include <cstring>
#include <vector>

#include "../../include/vr180_remap.h"
#include "../../vr180_convert_amd/csrc/jpeg_host.hpp"

using namespace v1c::jpeg;

namespace {

// the transform kernel's work on one block: rows, then columns, quantised into zigzag order
void transform_block(const uint8_t* img, int64_t pitch, const Geom& g, const Tables& t, uint32_t b, int16_t* zz)
{
    const BlockPos pos = block_pos(g, b);
    int tile[8][8];
    for (int r = 0; r < 8; r++) {
        int d[8];
        for (int c = 0; c < 8; c++)
            d[c] = plane_sample(img, pitch, g, pos.comp, pos.x0 + c, pos.y0 + r) - 128;
        fdct_pass<true>(d);
        for (int c = 0; c < 8; c++)
            tile[r][c] = d[c];
    }
    for (int c = 0; c < 8; c++) {
        int d[8];
        for (int i = 0; i < 8; i++)
            d[i] = tile[i][c];
        fdct_pass<false>(d);
        for (int i = 0; i < 8; i++)
            zz[zigzag_of(i * 8 + c)] = (int16_t)quantise(d[i], t.q[pos.comp ? 1 : 0][i * 8 + c]);
    }
}

struct Block {
    const int16_t* p;
    int operator()(int k) const { return p[k]; }
};

struct BitWriter {
    std::vector<uint8_t>& out;
    uint64_t bit;
    void operator()(uint32_t bits, int len)
    {
        for (int i = len - 1; i >= 0; i--, bit++) {
            if (out.size() <= bit >> 3)
                out.push_back(0);
            out[bit >> 3] |= (uint8_t)(((bits >> i) & 1u) << (7 - (bit & 7)));
        }
    }
};

}  // namespace

extern "C" {

uint64_t jpeg_emul_bound(int h, int w, int cn, int subsampling, int restart_mcus)
{
    Geom g;
    return make_geom(h, w, cn, subsampling, restart_mcus, g) ? scan_bound(g) : 0;
}

int jpeg_emul_zigzag(int natural)
{
    return zigzag_of(natural);
}

// coef: nblocks x 64; bits: nblocks; file: the whole file, `capacity` bytes.  Returns 0, -1 for invalid arguments, -2 where the file
// does not fit.
int jpeg_emul_encode(const uint8_t* img, int h, int w, int64_t pitch, int cn, int quality, int subsampling, int restart_mcus, int16_t* coef,
                     uint32_t* bits, uint8_t* file, uint64_t capacity, uint64_t* size_out)
{
    Geom g;
    if (quality < 1 || quality > 100 || !make_geom(h, w, cn, subsampling, restart_mcus, g))
        return -1;
    Tables t;
    make_tables(quality, t);
    for (uint32_t b = 0; b < g.nblocks; b++)
        transform_block(img, pitch, g, t, b, coef + (size_t)b * 64);
    std::vector<uint8_t> scan;
    for (uint32_t i = 0; i < g.nint; i++) {
        std::vector<uint8_t> raw;
        BitWriter bw{raw, 0};
        const uint32_t f = i * g.ibl, e = std::min(f + g.ibl, g.nblocks);
        for (uint32_t b = f; b < e; b++) {
            const uint32_t p = dc_predecessor(g, b);
            const int pred = p == b ? 0 : coef[(size_t)p * 64];
            const int tc = block_pos(g, b).comp ? 1 : 0;
            uint32_t n = 0;
            encode_block(Block{coef + (size_t)b * 64}, pred, t.dc[tc], t.ac[tc], [&](uint32_t, int len) { n += (uint32_t)len; });
            bits[b] = n;
            const uint64_t before = bw.bit;
            encode_block(Block{coef + (size_t)b * 64}, pred, t.dc[tc], t.ac[tc], bw);
            if (bw.bit - before != n)
                return -3;
        }
        const int pad = (int)((8 - (bw.bit & 7)) & 7);
        if (pad)
            bw((1u << pad) - 1u, pad);
        for (uint8_t v : raw) {
            scan.push_back(v);
            if (v == 0xff)
                scan.push_back(0);
        }
        if (i + 1 < g.nint) {
            scan.push_back(0xff);
            scan.push_back((uint8_t)(0xd0 + (i & 7)));
        }
    }
    if (scan.size() > scan_bound(g))
        return -4;
    const std::vector<uint8_t> head = file_header(g, quality);
    const uint64_t total = head.size() + scan.size() + 2;
    if (total > capacity)
        return -2;
    std::memcpy(file, head.data(), head.size());
    std::memcpy(file + head.size(), scan.data(), scan.size());
    file[total - 2] = 0xff, file[total - 1] = 0xd9;
    *size_out = total;
    return 0;
}

}
