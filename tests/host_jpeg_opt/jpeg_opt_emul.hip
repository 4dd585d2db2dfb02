// jpeg_opt_emul.hip -- TEST HARNESS: the optimised Huffman tables of the device JPEG encoder on the CPU: the product's symbol walk
// (jpeg_core.hpp: block_symbols) and table builder (jpeg_opt_core.hpp: build_table, on one lane) between the transform and the entropy
// coder of tests/host_jpeg/jpeg_emul.hip, which this file includes for its block transform and bit writer.
//
// Built by tests/test_jpeg_opt_host.py itself (hipcc --cuda-host-only -O2 -shared -fPIC, into a temporary directory) and compared there
// with the restatement (tests/jpg_opt_ref.py).  With -DJPEG_OPT_EMUL_MAIN it is a program of its own for a sanitizer build: it encodes
// the raw image files named on its command line.  Not part of the product: nothing in vr180_convert_amd/ loads it.
#include "../host_jpeg/jpeg_emul.hip"

#include "../../vr180_convert_amd/csrc/jpeg_opt_core.hpp"

extern "C" {

// the builder alone: the table of nsym counts; body: BITS, then HUFFVAL; codes: nsym entries.  Returns the bytes of body.
uint32_t jpeg_opt_emul_table(const uint64_t* counts, int nsym, uint32_t* codes, uint8_t* body)
{
    BuildScratch scratch;
    uint32_t len = 0;
    build_table(counts, nsym, scratch, codes, body, &len, OneLane{});
    return len;
}

// hist: 4 x 256 counts; codes: the code halves of the Tables the coder ran with (2 x 16, then 2 x 256 entries); file: the whole file.
// Returns 0, -1 for invalid arguments, -2 where the file does not fit, -3 where a block's size and its tokens disagree, -4 where the
// scan passes the bound.
int jpeg_opt_emul_encode(const uint8_t* img, int h, int w, int64_t pitch, int cn, int quality, int subsampling, int restart_mcus, uint64_t* hist,
                         uint32_t* codes, uint8_t* file, uint64_t capacity, uint64_t* size_out)
{
    Geom g;
    if (quality < 1 || quality > 100 || !make_geom(h, w, cn, subsampling, restart_mcus, g))
        return -1;
    Tables t;
    make_tables(quality, t);
    std::vector<int16_t> coef((size_t)g.nblocks * 64);
    for (uint32_t b = 0; b < g.nblocks; b++)
        transform_block(img, pitch, g, t, b, coef.data() + (size_t)b * 64);
    // the histogram kernel's work, block by block
    Hist hs{};
    uint32_t identity[256];
    for (int i = 0; i < 256; i++)
        identity[i] = identity_entry(i);
    for (uint32_t b = 0; b < g.nblocks; b++) {
        const uint32_t p = dc_predecessor(g, b);
        const int pred = p == b ? 0 : coef[(size_t)p * 64];
        const int tc = block_pos(g, b).comp ? 1 : 0;
        block_symbols(Block{coef.data() + (size_t)b * 64}, pred, identity, [&](bool dc, int symbol) { hs.n[hist_of(dc, tc)][symbol]++; });
    }
    // the builder kernel's, table by table
    DhtRecord rec{};
    BuildScratch scratch;
    for (int k = 0; k < (g.nc == 1 ? 2 : 4); k++)
        build_table(hs.n[k], (k & 1) ? 256 : 16, scratch, (k & 1) ? t.ac[k >> 1] : t.dc[k >> 1], rec.body[k], &rec.len[k], OneLane{});
    std::memcpy(hist, hs.n, sizeof(hs.n));
    std::memcpy(codes, t.dc, sizeof(t.dc));
    std::memcpy(codes + 32, t.ac, sizeof(t.ac));
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
            bool fits = true;
            encode_block(Block{coef.data() + (size_t)b * 64}, pred, t.dc[tc], t.ac[tc], [&](uint32_t, int len) {
                n += (uint32_t)len;
                fits = fits && len >= 1 && len <= 26;  // a symbol without a code has length 0
            });
            const uint64_t before = bw.bit;
            encode_block(Block{coef.data() + (size_t)b * 64}, pred, t.dc[tc], t.ac[tc], bw);
            if (bw.bit - before != n || !fits || n > 8u * kMaxBlockBytes)
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
    uint8_t dht[4 * (1 + kDhtTableMax)];
    const uint32_t dht_size = dht_body(rec, dht);
    const std::vector<uint8_t> head = file_header(g, quality, dht, dht_size);
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

#ifdef JPEG_OPT_EMUL_MAIN
#include <cstdio>
#include <cstdlib>
#include <string>

// arguments in groups of eight: raw-file h w cn pitch quality subsampling restart_mcus; writes raw-file.jpg
int main(int argc, char** argv)
{
    for (int a = 1; a + 8 <= argc; a += 8) {
        const int h = atoi(argv[a + 1]), w = atoi(argv[a + 2]), cn = atoi(argv[a + 3]), quality = atoi(argv[a + 5]);
        const int64_t pitch = atoll(argv[a + 4]);
        const int sub = atoi(argv[a + 6]), restart = atoi(argv[a + 7]);
        FILE* f = fopen(argv[a], "rb");
        if (!f)
            return 2;
        std::vector<uint8_t> img((size_t)h * pitch);
        if (fread(img.data(), 1, img.size(), f) != img.size())
            return 2;
        fclose(f);
        std::vector<uint64_t> hist(4 * 256);
        std::vector<uint32_t> codes(32 + 512);
        std::vector<uint8_t> file(jpeg_emul_bound(h, w, cn, sub, restart) + 4096);
        uint64_t size = 0;
        const int rc = jpeg_opt_emul_encode(img.data(), h, w, pitch, cn, quality, sub, restart, hist.data(), codes.data(), file.data(), file.size(), &size);
        if (rc != 0) {
            fprintf(stderr, "%s: %d\n", argv[a], rc);
            return 1;
        }
        const std::string out = std::string(argv[a]) + ".jpg";
        f = fopen(out.c_str(), "wb");
        if (!f || fwrite(file.data(), 1, size, f) != size)
            return 2;
        fclose(f);
        printf("%s: %llu bytes\n", out.c_str(), (unsigned long long)size);
    }
    return 0;
}
#endif
