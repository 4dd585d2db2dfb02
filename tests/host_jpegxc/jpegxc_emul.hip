// jpegxc_emul.hip -- TEST HARNESS: the lossless JPEG transcoder on the CPU: the product's checks and header writer (jpegxc_host.hpp), its
// per-block arithmetic (jpegxc_core.hpp: the source block of an output's block, the DC as a value, the range the encoder codes) and
// the encoder's entropy coder and optimised tables (jpeg_core.hpp, jpeg_batch.hpp, jpeg_opt_core.hpp) in a sequential copy of the
// kernels' passes, behind the decoder's sequential copy of tests/host_jpegdec/jpegdec_emul.hip, which this file includes for its
// decode up to the coefficients.
//
// Built by tests/test_jpegxc_host.py itself (hipcc --cuda-host-only -O2 -shared -fPIC, into a temporary directory) and compared there
// with the restatement (tests/jpgxc_ref.py).  With -DJXC_MAIN it is a stand-alone program that transcodes the cases of a manifest --
// the form the sanitizer run takes.  Not part of the product: nothing in vr180_convert_amd/ loads it.
#include "../host_jpegdec/jpegdec_emul.hip"

#include "../../vr180_convert_amd/csrc/jpeg_batch.hpp"
#include "../../vr180_convert_amd/csrc/jpeg_opt_core.hpp"
#include "../../vr180_convert_amd/csrc/jpegxc_host.hpp"

namespace jx = v1c::jpegxc;
namespace je = v1c::jpeg;

namespace {

uint32_t g_error_bit = 0xffffffffu;  // of the last call: the bit, where the last pass of a decode refused it (the composer's harness sets it too)

// An output as the harness takes it: width, height, restart_mcus, optimize, nregions, then six words per region.  Returns the words
// read, or 0 where the list ends early.
size_t read_output(const int32_t* spec, size_t left, v1c_jpeg_xc_output& o, std::vector<v1c_jpeg_xc_region>& regions)
{
    if (left < 5 || spec[4] < 0 || (size_t)spec[4] > (left - 5) / 6)
        return 0;
    std::memset(&o, 0, sizeof(o));
    o.width = spec[0], o.height = spec[1], o.restart_mcus = spec[2], o.optimize = spec[3], o.nregions = spec[4];
    regions.resize((size_t)o.nregions);
    for (int i = 0; i < o.nregions; i++) {
        const int32_t* r = spec + 5 + 6 * (size_t)i;
        regions[(size_t)i] = v1c_jpeg_xc_region{r[0], r[1], r[2], r[3], r[4], r[5]};
    }
    o.regions = regions.data();
    return 5 + 6 * (size_t)o.nregions;
}

struct XBlock {
    const int16_t* p;
    int operator()(int k) const { return p[k]; }
};

struct XBits {
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

// the encoder's passes behind the transform over one output's coefficients: (histograms, tables,) sizes, packing, stuffing, markers
int encode_coef(const je::Geom& g, const std::vector<int16_t>& coef, bool optimize, je::Tables& t, std::vector<uint8_t>& dht, std::vector<uint8_t>& scan)
{
    if (optimize) {
        je::Hist hs{};
        uint32_t identity[256];
        for (int i = 0; i < 256; i++)
            identity[i] = je::identity_entry(i);
        for (uint32_t b = 0; b < g.nblocks; b++) {
            const int tc = jx::table_class(g, b);
            je::block_symbols(XBlock{coef.data() + (size_t)b * 64}, jx::xc_prediction(g, coef.data(), 0, b), identity,
                              [&](bool dc, int symbol) { hs.n[je::hist_of(dc, tc)][symbol]++; });
        }
        je::DhtRecord rec{};
        je::BuildScratch scratch;
        for (int k = 0; k < (g.nc == 1 ? 2 : 4); k++)
            je::build_table(hs.n[k], (k & 1) ? 256 : 16, scratch, (k & 1) ? t.ac[k >> 1] : t.dc[k >> 1], rec.body[k], &rec.len[k], je::OneLane{});
        dht.resize(4 * (1 + je::kDhtTableMax));
        dht.resize(je::dht_body(rec, dht.data()));
    }
    for (uint32_t i = 0; i < g.nint; i++) {
        std::vector<uint8_t> raw;
        XBits bw{raw, 0};
        const uint32_t f = i * g.ibl, e = std::min(f + g.ibl, g.nblocks);
        for (uint32_t b = f; b < e; b++) {
            const int pred = jx::xc_prediction(g, coef.data(), 0, b);
            const int tc = jx::table_class(g, b);
            uint32_t n = 0;
            bool fits = true;
            je::encode_block(XBlock{coef.data() + (size_t)b * 64}, pred, t.dc[tc], t.ac[tc], [&](uint32_t, int len) {
                n += (uint32_t)len;
                fits = fits && len >= 1 && len <= 26;  // a symbol without a code has length 0
            });
            const uint64_t before = bw.bit;
            je::encode_block(XBlock{coef.data() + (size_t)b * 64}, pred, t.dc[tc], t.ac[tc], bw);
            if (bw.bit - before != n || !fits || n > 8u * je::kMaxBlockBytes)
                return -103;
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
            scan.push_back(je::rst_marker(i));
        }
    }
    return scan.size() > je::scan_bound(g) ? -104 : 0;
}

// The whole call.  Returns V1C_OK or the product's code for what it refuses (V1C_E_CORRUPT also for what the last pass finds), -100 for
// a malformed list of outputs, -101 where the decoder's decomposition disagrees with its parse, -102 where the files do not fit, -103 /
// -104 where a block or a scan passes its bound.  files: every output's file back to back; sizes: per output the header's bytes and the
// file's.
int transcode(const uint8_t* file, uint64_t size, uint32_t S, const int32_t* spec, size_t nspec, int n, uint8_t* files, uint64_t capacity,
              uint64_t* sizes)
{
    g_error_bit = 0xffffffffu;
    if (n < 1 || n > V1C_JPEG_XC_MAX_OUTPUTS)
        return V1C_E_INVALID;
    std::vector<v1c_jpeg_xc_output> outs((size_t)n);
    std::vector<std::vector<v1c_jpeg_xc_region>> regions((size_t)n);
    for (int i = 0; i < n; i++) {
        const size_t used = read_output(spec, nspec, outs[(size_t)i], regions[(size_t)i]);
        if (!used)
            return -100;
        spec += used, nspec -= used;
    }
    // every check of the product, in its order, before anything is decoded
    Run r;
    std::string why;
    if (!file)
        return V1C_E_INVALID;
    const ParseResult pr = parse(file, size, r.ps);
    if (pr != kParsed)
        return pr == kUnsupported ? V1C_E_UNSUPPORTED : V1C_E_CORRUPT;
    int rc = jx::source_error(r.ps, why);
    if (rc != V1C_OK)
        return rc;
    std::vector<je::Geom> geoms((size_t)n);
    std::vector<jx::RegionList> lists((size_t)n);
    for (int i = 0; i < n; i++) {
        rc = jx::check_output(r.ps.g, outs[(size_t)i], geoms[(size_t)i], lists[(size_t)i], why);
        if (rc != V1C_OK)
            return rc;
    }
    Run d;
    rc = run(file, size, S ? S : kDefaultSubseqBits, d);
    if (rc == 3) {
        g_error_bit = d.err;
        return V1C_E_CORRUPT;
    }
    if (rc != 0)
        return -101;
    const Geom& sg = d.ps.g;
    // the DC scan: differences by component, their exclusive sums
    std::vector<uint32_t> dcd(sg.nblocks);
    for (uint32_t b = 0; b < sg.nblocks; b++) {
        uint32_t pos, pos0;
        dc_pos(sg, b, pos, pos0);
        dcd[pos] = (uint32_t)(int)d.coef[(size_t)b * 64];
    }
    std::vector<uint64_t> dcoff(sg.nblocks + 1, 0);
    for (uint32_t b = 0; b < sg.nblocks; b++)
        dcoff[b + 1] = dcoff[b] + dcd[b];
    uint64_t at = 0;
    for (int i = 0; i < n; i++) {
        const je::Geom& g = geoms[(size_t)i];
        // the gather, block by block
        std::vector<int16_t> coef((size_t)g.nblocks * 64, 0);
        bool ok = true;
        for (uint32_t b = 0; b < g.nblocks; b++) {
            const uint32_t sb = jx::source_block(lists[(size_t)i], sg.mcux, g.mcux, sg.bpm, b);
            if (sb == jx::kNone)
                return -101;
            int16_t* dst = coef.data() + (size_t)b * 64;
            std::memcpy(dst, d.coef.data() + (size_t)sb * 64, 128);
            const int dc = jx::dc_value(sg, dcoff.data(), sb);  // (judged before it is cut to the 16 bits stored)
            dst[0] = (int16_t)(uint16_t)dc;
            ok &= jx::codable(dc, true);
            for (int k = 1; k < 64; k++)
                ok &= jx::codable(dst[k], false);
        }
        if (!ok)
            return V1C_E_UNSUPPORTED;
        je::Tables t;
        je::make_tables(50, t);  // (the code halves: Annex K; no stage behind the transform reads the quantiser half)
        std::vector<uint8_t> dht, scan;
        rc = encode_coef(g, coef, outs[(size_t)i].optimize != 0, t, dht, scan);
        if (rc != 0)
            return rc;
        const std::vector<uint8_t> head =
            jx::xc_header(d.ps, g, outs[(size_t)i].restart_mcus, dht.empty() ? nullptr : dht.data(), (uint32_t)dht.size());
        if (head.size() > V1C_JPEG_HEADER_XC_MAX || (!dht.empty() && !jx::whole_tables(dht.data(), (uint32_t)dht.size(), sg.nc)))
            return -104;
        const uint64_t total = head.size() + scan.size() + 2;
        if (at + total > capacity)
            return -102;
        std::memcpy(files + at, head.data(), head.size());
        std::memcpy(files + at + head.size(), scan.data(), scan.size());
        files[at + total - 2] = 0xff, files[at + total - 1] = 0xd9;
        sizes[2 * i] = head.size(), sizes[2 * i + 1] = total;
        at += total;
    }
    return V1C_OK;
}

}  // namespace

extern "C" {

int jxc_emul_transcode(const uint8_t* file, uint64_t size, uint32_t S, const int32_t* spec, uint64_t nspec, int n, uint8_t* files,
                       uint64_t capacity, uint64_t* sizes)
{
    return transcode(file, size, S, spec, (size_t)nspec, n, files, capacity, sizes);
}

// the bit of the unstuffed scan that the last call's V1C_E_CORRUPT of a last pass names
uint32_t jxc_emul_error_bit() { return g_error_bit; }

// the source block of every block of an output of dst_mcux x dst_mcuy MCUs (kNone where no region holds it): nregions x 6 words
void jxc_emul_source_blocks(const int32_t* regions, int nregions, uint32_t src_mcux, uint32_t dst_mcux, uint32_t dst_mcuy, uint32_t bpm, uint32_t* out)
{
    jx::RegionList l{};
    l.n = (uint32_t)nregions;
    for (int i = 0; i < nregions && i < (int)jx::kMaxRegions; i++)
        l.r[i] = jx::Region{(uint32_t)regions[6 * i], (uint32_t)regions[6 * i + 1], (uint32_t)regions[6 * i + 2], (uint32_t)regions[6 * i + 3],
                            (uint32_t)regions[6 * i + 4], (uint32_t)regions[6 * i + 5]};
    for (uint32_t b = 0; b < dst_mcux * dst_mcuy * bpm; b++)
        out[b] = jx::source_block(l, src_mcux, dst_mcux, bpm, b);
}

}

#ifdef JXC_MAIN
#include <cstdlib>
#include <fstream>
#include <sstream>

// Reads a manifest: one case per line, "<file> <expected return code> <n> <the outputs' words ...>".  Transcodes every case at two
// subsequence sizes and prints one line per case; the exit status is 0 unless a file cannot be read or a return code is not the
// expected one.
int main(int argc, char** argv)
{
    if (argc != 2)
        return 2;
    std::ifstream manifest(argv[1]);
    std::string line;
    int bad = 0;
    while (std::getline(manifest, line)) {
        std::istringstream in(line);
        std::string path;
        int want = 0, n = 0;
        if (!(in >> path >> want >> n))
            continue;
        std::vector<int32_t> spec;
        for (long v; in >> v;)
            spec.push_back((int32_t)v);
        std::FILE* f = std::fopen(path.c_str(), "rb");
        if (!f) {
            bad = 1;
            continue;
        }
        std::vector<uint8_t> data;
        uint8_t buf[4096];
        for (size_t k; (k = std::fread(buf, 1, sizeof(buf), f)) > 0;)
            data.insert(data.end(), buf, buf + k);
        std::fclose(f);
        // (exact-size heap copies: a read one byte past the file or the list is a sanitizer report)
        std::vector<uint8_t> exact(data.begin(), data.end());
        exact.shrink_to_fit();
        std::vector<int32_t> words(spec.begin(), spec.end());
        words.shrink_to_fit();
        for (uint32_t S : {256u, 1024u}) {
            std::vector<uint8_t> files((size_t)1 << 22);
            std::vector<uint64_t> sizes(2 * (size_t)(n > 0 ? n : 1) + 2, 0);
            const uint8_t* bytes = exact.empty() ? (const uint8_t*)"" : exact.data();  // (an empty file is a file, not a NULL pointer)
            const int rc = transcode(bytes, exact.size(), S, words.data(), words.size(), n, files.data(), files.size(), sizes.data());
            unsigned long sum = 0, total = 0;
            for (int i = 0; rc == 0 && i < n; i++)
                total += sizes[2 * i + 1];
            for (unsigned long i = 0; i < total; i++)
                sum += files[i];
            std::printf("%s S=%u rc=%d want=%d bytes=%lu sum=%lu\n", path.c_str(), S, rc, want, total, sum);
            if (rc != want)
                bad = 1;
        }
    }
    return bad;
}
#endif
