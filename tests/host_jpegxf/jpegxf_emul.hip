// jpegxf_emul.hip -- TEST HARNESS: the lossless JPEG composer on the CPU: the product's checks and header writer (jpegxf_host.hpp) and
// its per-block arithmetic (jpegxf_core.hpp: the source block of an output's block, the source coefficient of a coefficient and its
// sign) in a sequential copy of the gather kernel's pass, behind the decoder's sequential copy and in front of the encoder's, both of
// tests/host_jpegxc/jpegxc_emul.hip, which this file includes.
//
// Built by tests/test_jpegxf_host.py itself (hipcc --cuda-host-only -O2 -shared -fPIC, into a temporary directory) and compared there
// with the restatement (tests/jpgxf_ref.py).  With -DJXF_MAIN it is a stand-alone program that composes the cases of a manifest -- the
// form the sanitizer run takes.  Not part of the product: nothing in vr180_convert_amd/ loads it.
#include "../host_jpegxc/jpegxc_emul.hip"

#include "../../vr180_convert_amd/csrc/jpegxf_host.hpp"

namespace jf = v1c::jpegxf;

namespace {

// An output as the harness takes it: width, height, restart_mcus, optimize, nregions, then eight words per region.  Returns the words
// read, or 0 where the list ends early.
size_t read_xf_output(const int32_t* spec, size_t left, v1c_jpeg_xf_output& o, std::vector<v1c_jpeg_xf_region>& regions)
{
    if (left < 5 || spec[4] < 0 || (size_t)spec[4] > (left - 5) / 8)
        return 0;
    std::memset(&o, 0, sizeof(o));
    o.width = spec[0], o.height = spec[1], o.restart_mcus = spec[2], o.optimize = spec[3], o.nregions = spec[4];
    regions.resize((size_t)o.nregions);
    for (int i = 0; i < o.nregions; i++) {
        const int32_t* r = spec + 5 + 8 * (size_t)i;
        regions[(size_t)i] = v1c_jpeg_xf_region{r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]};
    }
    o.regions = regions.data();
    return 5 + 8 * (size_t)o.nregions;
}

// The whole call over the files blob[0 ... sizes[0]), blob[sizes[0] ...), ...  Returns V1C_OK or the product's code for what it refuses
// (V1C_E_CORRUPT also for what the last pass of a decode finds; *damaged: that source), and the transcoder's harness's negative codes
// for its own troubles.  files: every output's file back to back; out_sizes: per output the header's bytes and the file's.
int compose(const uint8_t* blob, const uint64_t* sizes, int nsources, uint32_t S, const int32_t* spec, size_t nspec, int n, uint8_t* files,
            uint64_t capacity, uint64_t* out_sizes, int* damaged)
{
    if (damaged)
        *damaged = -1;
    g_error_bit = 0xffffffffu;
    if (nsources < 1 || nsources > V1C_JPEG_XF_MAX_SOURCES || n < 1 || n > V1C_JPEG_XC_MAX_OUTPUTS)
        return V1C_E_INVALID;
    std::vector<v1c_jpeg_xf_output> outs((size_t)n);
    std::vector<std::vector<v1c_jpeg_xf_region>> regions((size_t)n);
    for (int i = 0; i < n; i++) {
        const size_t used = read_xf_output(spec, nspec, outs[(size_t)i], regions[(size_t)i]);
        if (!used)
            return -100;
        spec += used, nspec -= used;
    }
    // every check of the product, in its order, before anything is decoded
    std::vector<const uint8_t*> file((size_t)nsources);
    std::vector<Parsed> ps((size_t)nsources);
    std::string why;
    uint64_t off = 0;
    for (int i = 0; i < nsources; i++) {
        file[(size_t)i] = blob + off, off += sizes[i];
        const ParseResult pr = parse(file[(size_t)i], sizes[i], ps[(size_t)i]);
        if (pr != kParsed)
            return pr == kUnsupported ? V1C_E_UNSUPPORTED : V1C_E_CORRUPT;
        const int rc = jx::source_error(ps[(size_t)i], why);
        if (rc != V1C_OK)
            return rc;
    }
    int rc = jf::sources_error(ps, why);
    if (rc != V1C_OK)
        return rc;
    std::vector<je::Geom> geoms((size_t)n);
    std::vector<jf::RegionList> lists((size_t)n);
    for (int i = 0; i < n; i++) {
        rc = jf::check_output(ps, outs[(size_t)i], geoms[(size_t)i], lists[(size_t)i], why);
        if (rc != V1C_OK)
            return rc;
    }
    // every source's decode and DC scan: differences by component, their exclusive sums
    std::vector<Run> d((size_t)nsources);
    std::vector<std::vector<uint64_t>> dcoff((size_t)nsources);
    for (int i = 0; i < nsources; i++) {
        rc = run(file[(size_t)i], sizes[i], S ? S : kDefaultSubseqBits, d[(size_t)i]);
        if (rc == 3) {
            g_error_bit = d[(size_t)i].err;
            if (damaged)
                *damaged = i;
            return V1C_E_CORRUPT;
        }
        if (rc != 0)
            return -101;
        const Geom& sg = d[(size_t)i].ps.g;
        std::vector<uint32_t> dcd(sg.nblocks);
        for (uint32_t b = 0; b < sg.nblocks; b++) {
            uint32_t pos, pos0;
            dc_pos(sg, b, pos, pos0);
            dcd[pos] = (uint32_t)(int)d[(size_t)i].coef[(size_t)b * 64];
        }
        dcoff[(size_t)i].assign(sg.nblocks + 1, 0);
        for (uint32_t b = 0; b < sg.nblocks; b++)
            dcoff[(size_t)i][b + 1] = dcoff[(size_t)i][b] + dcd[b];
    }
    const Geom& g0 = ps[0].g;
    uint64_t at = 0;
    for (int i = 0; i < n; i++) {
        const je::Geom& g = geoms[(size_t)i];
        // the gather, block by block and coefficient by coefficient
        std::vector<int16_t> coef((size_t)g.nblocks * 64, 0);
        bool ok = true;
        for (uint32_t b = 0; b < g.nblocks; b++) {
            const jf::SourceBlock sb = jf::source_block(lists[(size_t)i], g.mcux, g0.hs, g0.vs, g0.bpm, b);
            if (sb.block == jf::kNone || sb.source >= (uint32_t)nsources || sb.block >= d[sb.source].ps.g.nblocks)
                return -101;
            const int16_t* src = d[sb.source].coef.data() + (size_t)sb.block * 64;
            int16_t* dst = coef.data() + (size_t)b * 64;
            const int dc = jx::dc_value(d[sb.source].ps.g, dcoff[sb.source].data(), sb.block);  // (judged before it is cut to the 16 bits stored)
            dst[0] = (int16_t)(uint16_t)dc;
            ok &= jx::codable(dc, true);
            const uint64_t neg = jf::negated(sb.code);
            for (uint32_t z = 1; z < 64; z++) {
                const int v = src[jf::source_coefficient(sb.code, z)], w = ((neg >> z) & 1u) ? -v : v;
                dst[z] = (int16_t)w;
                ok &= jx::codable(w, false);
            }
        }
        if (!ok)
            return V1C_E_UNSUPPORTED;
        je::Tables t;
        je::make_tables(50, t);  // (the code halves: Annex K; no stage behind the transform reads the quantiser half)
        std::vector<uint8_t> dht, scan;
        rc = encode_coef(g, coef, outs[(size_t)i].optimize != 0, t, dht, scan);
        if (rc != 0)
            return rc;
        const jf::Region& r0 = lists[(size_t)i].r[0];
        const std::vector<uint8_t> head = jf::xf_header(ps[r0.source], (r0.code & jf::kTranspose) != 0, g, outs[(size_t)i].restart_mcus,
                                                        dht.empty() ? nullptr : dht.data(), (uint32_t)dht.size());
        if (head.size() > V1C_JPEG_HEADER_XC_MAX || (!dht.empty() && !jx::whole_tables(dht.data(), (uint32_t)dht.size(), g0.nc)))
            return -104;
        const uint64_t total = head.size() + scan.size() + 2;
        if (at + total > capacity)
            return -102;
        std::memcpy(files + at, head.data(), head.size());
        std::memcpy(files + at + head.size(), scan.data(), scan.size());
        files[at + total - 2] = 0xff, files[at + total - 1] = 0xd9;
        out_sizes[2 * i] = head.size(), out_sizes[2 * i + 1] = total;
        at += total;
    }
    return V1C_OK;
}

}  // namespace

extern "C" {

int jxf_emul_compose(const uint8_t* blob, const uint64_t* sizes, int nsources, uint32_t S, const int32_t* spec, uint64_t nspec, int n, uint8_t* files,
                     uint64_t capacity, uint64_t* out_sizes, int* damaged)
{
    return compose(blob, sizes, nsources, S, spec, (size_t)nspec, n, files, capacity, out_sizes, damaged);
}

// jpegxf_core.hpp's tables: from[code * 64 + z] the source's zigzag position of the result's position z, masks[code] the negated
// positions; returns whether its zigzag order is the encoder's (jpeg_core.hpp: zigzag_of)
int jxf_emul_tables(uint8_t* from, uint64_t* masks)
{
    int same = 1;
    for (int n = 0; n < 64; n++)
        same &= jf::detail::zz(n) == je::zigzag_of(n);
    for (uint32_t code = 0; code < 8; code++) {
        masks[code] = jf::negated(code);
        for (uint32_t z = 0; z < 64; z++)
            from[code * 64 + z] = (uint8_t)jf::source_coefficient(code, z);
    }
    return same;
}

// (source, code, block) of every block of an output of dst_mcux x dst_mcuy MCUs (block kNone where no region holds it): nregions x 9
// words as jpegxf_core.hpp's Region
void jxf_emul_source_blocks(const uint32_t* regions, int nregions, uint32_t dst_mcux, uint32_t dst_mcuy, uint32_t hs, uint32_t vs, uint32_t bpm,
                            uint32_t* out)
{
    jf::RegionList l{};
    l.n = (uint32_t)nregions;
    for (int i = 0; i < nregions && i < (int)jf::kMaxRegions; i++) {
        const uint32_t* r = regions + 9 * i;
        l.r[i] = jf::Region{r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8]};
    }
    for (uint32_t b = 0; b < dst_mcux * dst_mcuy * bpm; b++) {
        const jf::SourceBlock s = jf::source_block(l, dst_mcux, hs, vs, bpm, b);
        out[3 * b] = s.source, out[3 * b + 1] = s.code, out[3 * b + 2] = s.block;
    }
}

}

#ifdef JXF_MAIN
#include <cstdlib>
#include <fstream>
#include <sstream>

// Reads a manifest: one case per line, "<expected return code> <nsources> <file> ... <n> <the outputs' words ...>".  Composes every
// case at two subsequence sizes and prints one line per case and size; the exit status is 0 unless a file cannot be read or a return
// code is not the expected one.
int main(int argc, char** argv)
{
    if (argc != 2)
        return 2;
    std::ifstream manifest(argv[1]);
    std::string line;
    int bad = 0;
    while (std::getline(manifest, line)) {
        std::istringstream in(line);
        int want = 0, nsources = 0, n = 0;
        if (!(in >> want >> nsources) || nsources < 0 || nsources > 16)
            continue;
        std::vector<uint8_t> blob;
        std::vector<uint64_t> sizes;
        bool read = true;
        for (int i = 0; i < nsources; i++) {
            std::string path;
            in >> path;
            std::FILE* f = std::fopen(path.c_str(), "rb");
            if (!f) {
                read = false;
                break;
            }
            const size_t before = blob.size();
            uint8_t buf[4096];
            for (size_t k; (k = std::fread(buf, 1, sizeof(buf), f)) > 0;)
                blob.insert(blob.end(), buf, buf + k);
            std::fclose(f);
            sizes.push_back(blob.size() - before);
        }
        if (!read || !(in >> n)) {
            bad = 1;
            continue;
        }
        std::vector<int32_t> spec;
        for (long v; in >> v;)
            spec.push_back((int32_t)v);
        // (exact-size heap copies: a read one byte past the last file or the list is a sanitizer report)
        std::vector<uint8_t> exact(blob.begin(), blob.end());
        exact.shrink_to_fit();
        std::vector<int32_t> words(spec.begin(), spec.end());
        words.shrink_to_fit();
        for (uint32_t S : {256u, 1024u}) {
            std::vector<uint8_t> files((size_t)1 << 22);
            std::vector<uint64_t> out_sizes(2 * (size_t)(n > 0 ? n : 1) + 2, 0);
            const uint8_t* bytes = exact.empty() ? (const uint8_t*)"" : exact.data();
            int damaged = -1;
            const int rc = compose(bytes, sizes.data(), nsources, S, words.data(), words.size(), n, files.data(), files.size(), out_sizes.data(), &damaged);
            unsigned long sum = 0, total = 0;
            for (int i = 0; rc == 0 && i < n; i++)
                total += out_sizes[2 * i + 1];
            for (unsigned long i = 0; i < total; i++)
                sum += files[i];
            std::printf("%s S=%u rc=%d want=%d bytes=%lu sum=%lu\n", line.substr(0, 60).c_str(), S, rc, want, total, sum);
            if (rc != want)
                bad = 1;
        }
    }
    return bad;
}
#endif
