// jpeg_batch_emul.hip -- TEST HARNESS: a sequential copy of the batched JPEG encoder's decomposition (kernels_jpeg_batch.hip, and
// encode_chunk of jpeg.hip) on the CPU, built from the product's headers: jpeg_core.hpp (the arithmetic), jpeg_host.hpp (tables and
// header segments) and jpeg_batch.hpp (regions, work lists, file_of, the values relative to an image, chunk_ends).  Every kernel is a
// loop over the workgroups of its work list and over 256 lanes; every workgroup finds its image with file_of and works with
// image-relative indices, as on the device; the scans run over the concatenated buffers.
//
// Built by tests/test_jpeg_batch_host.py itself (hipcc --cuda-host-only, into a temporary directory): as a shared library; with
// -DJPEGB_MAIN as a program of its own for the sanitizer run; with -DJPEGB_BREAK=1 / 2 / 3 broken on purpose (switches of this
// harness only: the product has none).  Not part of the product: nothing in vr180_convert_amd/ loads it.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/vr180_remap.h"
#include "../../vr180_convert_amd/csrc/jpeg_batch.hpp"
#include "../../vr180_convert_amd/csrc/jpeg_host.hpp"

#ifndef JPEGB_BREAK
#define JPEGB_BREAK 0
#endif

using namespace v1c::jpeg;

extern "C" {
struct EmulImage {
    const uint8_t* img;
    int32_t h, w;
    int64_t pitch;
    int32_t cn, quality, subsampling, restart_mcus;
    int16_t* coef;   // nblocks x 64
    uint32_t* bits;  // nblocks
    uint8_t* file;   // the whole file
    uint64_t capacity;
    uint64_t size;   // out
};
}

namespace {

// k_jpegb_transform's work on one block
void transform_block(const Image& im, const Tables& t, uint32_t b, int16_t* zz)
{
    const BlockPos pos = block_pos(im.g, b);
    int tile[8][8];
    for (int r = 0; r < 8; r++) {
        int d[8];
        for (int c = 0; c < 8; c++)
            d[c] = plane_sample(im.img, im.pitch, im.g, pos.comp, pos.x0 + c, pos.y0 + r) - 128;
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

// the kernels' Packer: a 64-bit accumulator, byte-swapped 32-bit words, ORs for a block's first and last word, plain stores between
struct Packer {
    uint32_t* w;
    unsigned long long acc = 0;
    int n;
    bool first = true;
    Packer(uint32_t* raw, uint64_t bit) : w(raw + (bit >> 5)), n((int)(bit & 31)) {}
    void operator()(uint32_t bits, int len)
    {
        acc = (acc << len) | bits;
        n += len;
        if (n >= 32) {
            n -= 32;
            const uint32_t word = __builtin_bswap32((uint32_t)(acc >> n));
            acc &= (1ull << n) - 1;
            if (first)
                *w |= word;
            else
                *w = word;
            first = false;
            w++;
        }
    }
    void finish()
    {
        if (n)
            *w |= __builtin_bswap32((uint32_t)(acc << (32 - n)));
    }
};

// launch_scan: out[i] = the sum of in[0 .. i), out[n] = the total
void scan(const std::vector<uint32_t>& in, std::vector<uint64_t>& out)
{
    out.assign(in.size() + 1, 0);
    for (size_t i = 0; i < in.size(); i++)
        out[i + 1] = out[i] + in[i];
}

int prediction(const Image& im, const int16_t* coef, uint32_t b)
{
#if JPEGB_BREAK == 1
    // the DC predecessor carried over an image boundary: the image's first MCU predicts from the blocks in front of it
    if (dc_predecessor(im.g, b) == b && b < im.g.bpm && im.blk0 > 0)
        return coef[(size_t)(im.blk0 + b - 1) * 64];
#endif
    return dc_prediction(im, coef, b);
}

struct Chunk {
    uint32_t n;
    std::vector<Image> im;
    std::vector<uint32_t> first;
    std::vector<Tables> tabs;
    Totals t;
};

const uint32_t* list_of(const Chunk& c, int list)
{
    return c.first.data() + (size_t)list * (c.n + 1);
}

// one chunk: images [lo, hi).  0, -2 where a file does not fit, or -3 where a block's packed bits are not the bits counted for it
int encode_chunk(EmulImage* images, const std::vector<Geom>& geoms, uint32_t lo, uint32_t hi)
{
    Chunk c;
    c.n = hi - lo;
    c.im.resize(c.n);
    c.first.assign((size_t)kWorkLists * (c.n + 1), 0);
    std::vector<int> quality;
    for (uint32_t f = 0; f < c.n; f++) {
        const EmulImage& v = images[lo + f];
        const auto it = std::find(quality.begin(), quality.end(), v.quality);
        c.im[f].img = v.img, c.im[f].pitch = v.pitch, c.im[f].g = geoms[lo + f], c.im[f].tab = (uint32_t)(it - quality.begin());
        if (it == quality.end())
            quality.push_back(v.quality);
    }
    c.tabs.resize(quality.size());
    for (size_t k = 0; k < quality.size(); k++)
        make_tables(quality[k], c.tabs[k]);
    c.t = place_regions(c.im.data(), c.n, c.first.data());
    const Totals& t = c.t;

    std::vector<int16_t> coef(t.nblocks * 64, (int16_t)0x5a5a);  // (not zero: what lies in front of an image must not matter)
    std::vector<uint32_t> bits(t.nblocks, 0xdeadbeefu), ibytes(t.nint, 0xdeadbeefu), raw(t.pieces * (kPiece / 4) + 4, 0), ffcnt(t.pieces, 0);
    std::vector<uint64_t> bitoff, ioff, ffoff, sizes(c.n, 0);
    std::vector<uint8_t> out(t.out_bytes + 8, 0xee);

    // 1: transform, 32 blocks per workgroup
    const uint32_t* first = list_of(c, kByTile);
    for (uint32_t g = 0; g < first[c.n]; g++) {
        const uint32_t f = file_of(first, c.n, g), wg = g - first[f];
        const Image& im = c.im[f];
        for (uint32_t blk = 0; blk < 32; blk++) {
            const uint32_t b = wg * 32 + blk;
            if (b < im.g.nblocks)
                transform_block(im, c.tabs[im.tab], b, coef.data() + (size_t)(im.blk0 + b) * 64);
        }
    }
    // 2: size, a block per lane
    first = list_of(c, kByBlock);
    for (uint32_t g = 0; g < first[c.n]; g++) {
        const uint32_t f = file_of(first, c.n, g), wg = g - first[f];
        const Image& im = c.im[f];
        const Tables& tab = c.tabs[im.tab];
        for (uint32_t tid = 0; tid < 256; tid++) {
            const uint32_t b = wg * 256 + tid;
            if (b >= im.g.nblocks)
                continue;
            const int tc = block_pos(im.g, b).comp ? 1 : 0;
            uint32_t n = 0;
            encode_block(Block{coef.data() + (size_t)(im.blk0 + b) * 64}, prediction(im, coef.data(), b), tab.dc[tc], tab.ac[tc],
                         [&](uint32_t, int len) { n += (uint32_t)len; });
            bits[im.blk0 + b] = n;
        }
    }
    scan(bits, bitoff);
    // 3: interval bytes, an interval per lane of the block list's workgroups
    for (uint32_t g = 0; g < first[c.n]; g++) {
        const uint32_t f = file_of(first, c.n, g), wg = g - first[f];
        const Image& im = c.im[f];
        for (uint32_t tid = 0; tid < 256; tid++) {
            const uint32_t i = wg * 256 + tid;
            if (i < im.g.nint)
                ibytes[im.int0 + i] = interval_bytes(im, bitoff.data(), i);
        }
    }
    scan(ibytes, ioff);
    // 4: pack
    for (uint32_t g = 0; g < first[c.n]; g++) {
        const uint32_t f = file_of(first, c.n, g), wg = g - first[f];
        const Image& im = c.im[f];
        const Tables& tab = c.tabs[im.tab];
        for (uint32_t tid = 0; tid < 256; tid++) {
            const uint32_t b = wg * 256 + tid;
            if (b >= im.g.nblocks)
                continue;
            const int tc = block_pos(im.g, b).comp ? 1 : 0;
            const uint64_t bit = block_bit(im, bitoff.data(), ioff.data(), b);
            Packer pk(raw.data() + (size_t)im.piece0 * (kPiece / 4), bit);
            encode_block(Block{coef.data() + (size_t)(im.blk0 + b) * 64}, prediction(im, coef.data(), b), tab.dc[tc], tab.ac[tc], pk);
            if (b + 1 == im.g.nblocks || (b + 1) % im.g.ibl == 0) {
                const int pad = (int)((8 - ((bit + bits[im.blk0 + b]) & 7)) & 7);
                if (pad)
                    pk((1u << pad) - 1u, pad);
            }
            pk.finish();
            const uint64_t end = 8 * (uint64_t)((const uint8_t*)pk.w - (const uint8_t*)(raw.data() + (size_t)im.piece0 * (kPiece / 4))) + pk.n;
            if (end < bit + bits[im.blk0 + b] || end > 8 * raw_bound(im.g))
                return -3;
        }
    }
    // 5: count, over the concatenation
    const uint8_t* rb = (const uint8_t*)raw.data();
    for (uint64_t p = 0; p < t.pieces; p++)
        for (int j = 0; j < kPiece; j++)
            ffcnt[p] += rb[p * kPiece + j] == 0xff;
    scan(ffcnt, ffoff);
    // 6: place, a piece per lane
    first = list_of(c, kByPiece);
    for (uint32_t g = 0; g < first[c.n]; g++) {
        const uint32_t f = file_of(first, c.n, g), wg = g - first[f];
        const Image& im = c.im[f];
        for (uint32_t tid = 0; tid < 256; tid++) {
            const uint64_t p = (uint64_t)wg * 256 + tid;
            const uint64_t total = interval_start(im, ioff.data(), im.g.nint), g0 = p * kPiece;
            if (p >= pieces_of(im.g) || g0 >= total)
                continue;
            uint32_t l = 0, h = im.g.nint - 1;
            while (l < h) {
                const uint32_t mid = (l + h + 1) >> 1;
                if (interval_start(im, ioff.data(), mid) <= g0)
                    l = mid;
                else
                    h = mid - 1;
            }
            uint32_t iv = l;
            uint64_t next = interval_start(im, ioff.data(), iv + 1);
#if JPEGB_BREAK == 3
            uint64_t ff = ffoff[im.piece0 + p];  // the image's base not subtracted
#else
            uint64_t ff = ff_before(im, ffoff.data(), p);
#endif
            uint8_t* o = out.data() + im.out0;
            for (int j = 0; j < kPiece; j++) {
                const uint64_t gb = g0 + j;
                if (gb >= total)
                    break;
                if (gb >= next) {
                    iv++;
                    next = interval_start(im, ioff.data(), iv + 1);
                }
                const uint32_t byte = rb[(im.piece0 + p) * kPiece + j];
                uint64_t at = gb + ff + 2ull * iv;
                if (im.out0 + at + 4 > out.size())
                    continue;  // (only a build broken on purpose gets here: outside the whole buffer)
                o[at++] = (uint8_t)byte;
                if (byte == 255u) {
                    o[at++] = 0;
                    ff++;
                }
                if (gb + 1 == next && iv + 1 < im.g.nint) {
                    o[at] = 0xff;
#if JPEGB_BREAK == 2
                    o[at + 1] = rst_marker((uint32_t)im.int0 + iv);  // RSTm numbered over the batch
#else
                    o[at + 1] = rst_marker(iv);
#endif
                }
                if (gb + 1 == total)
                    sizes[f] = at;
            }
        }
    }
    // the host's part: header, scan, EOI; and the intermediate results for the test
    for (uint32_t f = 0; f < c.n; f++) {
        EmulImage& v = images[lo + f];
        const Image& im = c.im[f];
        v.size = 0;
        if (sizes[f] == 0 || sizes[f] > scan_bound(im.g))
            continue;  // (a size outside its bound: the file is left empty, which no reference is)
        std::memcpy(v.coef, coef.data() + (size_t)im.blk0 * 64, (size_t)im.g.nblocks * 128);
        std::memcpy(v.bits, bits.data() + im.blk0, (size_t)im.g.nblocks * 4);
        const std::vector<uint8_t> head = file_header(im.g, v.quality);
        const uint64_t total = head.size() + sizes[f] + 2;
        if (total > v.capacity)
            return -2;
        std::memcpy(v.file, head.data(), head.size());
        std::memcpy(v.file + head.size(), out.data() + im.out0, sizes[f]);
        v.file[total - 2] = 0xff, v.file[total - 1] = 0xd9;
        v.size = total;
    }
    return 0;
}

}  // namespace

extern "C" {

uint64_t jpegb_emul_workspace(int h, int w, int cn, int subsampling, int restart_mcus)
{
    Geom g;
    return make_geom(h, w, cn, subsampling, restart_mcus, g) ? workspace_of(g) : 0;
}

uint64_t jpegb_emul_default_budget()
{
    return kDefaultBatchWorkspace;
}

uint32_t jpegb_emul_file_of(const uint32_t* first, uint32_t n, uint32_t wg)
{
    return file_of(first, n, wg);
}

// the work lists (kWorkLists * (n + 1) words) and the regions (blk0, int0, piece0, out0, then nblocks, nint, pieces, scan bound, per
// image) of the list as ONE chunk
int jpegb_emul_tables(int n, const EmulImage* images, uint32_t* first, uint64_t* regions)
{
    std::vector<Image> im((size_t)n);
    for (int i = 0; i < n; i++)
        if (!make_geom(images[i].h, images[i].w, images[i].cn, images[i].subsampling, images[i].restart_mcus, im[i].g))
            return -1;
    place_regions(im.data(), (uint32_t)n, first);
    for (int i = 0; i < n; i++) {
        const uint64_t r[8] = {im[i].blk0, im[i].int0, im[i].piece0, im[i].out0, im[i].g.nblocks, im[i].g.nint, pieces_of(im[i].g), scan_bound(im[i].g)};
        std::memcpy(regions + (size_t)i * 8, r, sizeof(r));
    }
    return kWorkLists;
}

// The batch, cut into chunks as v1c_jpeg_encode_batch cuts it.  Returns 0, -1 for invalid arguments, -2 where a file does not fit,
// -3 for an inconsistency; a file whose size left its bound has size 0.
int jpegb_emul_encode(int n, EmulImage* images, uint64_t budget, uint32_t* chunks_out)
{
    if (chunks_out)
        *chunks_out = 0;
    if (n < 0 || (n && !images))
        return -1;
    std::vector<Geom> geoms((size_t)n);
    std::vector<uint64_t> bytes, groups;
    for (int i = 0; i < n; i++) {
        const EmulImage& v = images[i];
        if (v.quality < 1 || v.quality > 100 || v.pitch < (int64_t)v.w * v.cn || !make_geom(v.h, v.w, v.cn, v.subsampling, v.restart_mcus, geoms[i]))
            return -1;
        bytes.push_back(workspace_of(geoms[i]));
        groups.push_back(most_groups(geoms[i]));
    }
    uint32_t lo = 0, chunk = 0;
    for (uint32_t hi : chunk_ends(bytes, groups, budget ? budget : kDefaultBatchWorkspace)) {
        const int rc = encode_chunk(images, geoms, lo, hi);
        if (rc)
            return rc;
        lo = hi, chunk++;
        if (chunks_out)
            *chunks_out = chunk;
    }
    return 0;
}

}

#ifdef JPEGB_MAIN
// jpeg_batch_emul LIST BUDGET...: LIST holds one image per line, "h w cn pitch quality subsampling restart offset file" with `file` the
// raw buffer the image lies in; runs the batch once per budget and prints every file's size and CRC-32.
static uint32_t crc32(const uint8_t* p, size_t n)
{
    uint32_t c = 0xffffffffu;
    for (size_t i = 0; i < n; i++) {
        c ^= p[i];
        for (int k = 0; k < 8; k++)
            c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
    }
    return ~c;
}

int main(int argc, char** argv)
{
    if (argc < 3)
        return 2;
    FILE* list = std::fopen(argv[1], "r");
    if (!list)
        return 2;
    std::vector<EmulImage> images;
    std::vector<std::vector<uint8_t>> bases;
    std::vector<uint64_t> offsets;
    char path[4096];
    EmulImage v{};
    long long pitch, offset;
    while (std::fscanf(list, "%d %d %d %lld %d %d %d %lld %4095s", &v.h, &v.w, &v.cn, &pitch, &v.quality, &v.subsampling, &v.restart_mcus, &offset,
                       path) == 9) {
        FILE* f = std::fopen(path, "rb");
        if (!f)
            return 2;
        std::vector<uint8_t> data;
        uint8_t buf[4096];
        for (size_t k; (k = std::fread(buf, 1, sizeof(buf), f)) > 0;)
            data.insert(data.end(), buf, buf + k);
        std::fclose(f);
        v.pitch = pitch;
        bases.push_back(std::move(data));
        offsets.push_back((uint64_t)offset);
        images.push_back(v);
    }
    std::fclose(list);
    const int n = (int)images.size();
    std::vector<std::vector<int16_t>> coef(n);
    std::vector<std::vector<uint32_t>> bits(n);
    std::vector<std::vector<uint8_t>> files(n);
    for (int i = 0; i < n; i++) {
        Geom g;
        if (!make_geom(images[i].h, images[i].w, images[i].cn, images[i].subsampling, images[i].restart_mcus, g))
            return 2;
        coef[i].resize((size_t)g.nblocks * 64), bits[i].resize(g.nblocks), files[i].resize(scan_bound(g) + V1C_JPEG_HEADER_MAX + 2);
        images[i].img = bases[i].data() + offsets[i];
        images[i].coef = coef[i].data(), images[i].bits = bits[i].data(), images[i].file = files[i].data(), images[i].capacity = files[i].size();
    }
    for (int a = 2; a < argc; a++) {
        const uint64_t budget = std::strtoull(argv[a], nullptr, 10);
        uint32_t chunks = 0;
        const int rc = jpegb_emul_encode(n, images.data(), budget, &chunks);
        std::printf("batch budget=%llu rc=%d chunks=%u\n", (unsigned long long)budget, rc, chunks);
        if (rc)
            return 1;
        for (int i = 0; i < n; i++)
            std::printf("image %d size=%llu crc=%08x\n", i, (unsigned long long)images[i].size, crc32(images[i].file, images[i].size));
    }
    return 0;
}
#endif
