// jpegprog_emul.hip -- TEST HARNESS: runs the product's progressive JPEG decoding (jpegprog_core.hpp: the lane functions of every
// kernel of kernels_jpegprog.hip; jpegprog_host.hpp: the parse over all scans) on the CPU, in a sequential copy of the kernels'
// decomposition: per scan the unstuffing by 16-byte pieces, the rounds over all subsequences with two exit buffers, the skip rule and
// the flag, the block-count scan, the last pass, the DC scan; behind the last scan the DC differences and the sequential decoder's
// pixel stage (jpegdec_core.hpp).
//
// Built by tests/test_jpegprog_host.py itself (hipcc --cuda-host-only -O2 -shared -fPIC, into a temporary directory) and compared there
// with the restatement (tests/jpgprog_ref.py).  With -DJPROG_MAIN it is a stand-alone program that decodes the files named on its
// command line -- the form the sanitizer run takes.  Not part of the product: nothing in vr180_convert_amd/ loads it.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/vr180_remap.h"
#include "../../vr180_convert_amd/csrc/jpegprog_host.hpp"

using namespace v1c::jpegdec;
namespace jp = v1c::jpegprog;

namespace {

struct Run {
    jp::PParsed ps;
    std::vector<int16_t> coef;
    std::vector<std::vector<int16_t>> after;  // the store behind every scan (keep)
    std::vector<jp::PState> entry;            // all scans' subsequences back to back
    std::vector<uint32_t> count, scan_rounds, scan_nsub;
    uint32_t err = jp::kNoError, err_scan = 0;
    bool keep = false;
};

// 0: decoded, 1: unsupported, 2: corrupt by the parse, 3: corrupt by the last pass, -1: the decomposition disagrees with the parse
int run(const uint8_t* file, uint64_t size, uint32_t S, Run& r)
{
    const ParseResult pr = jp::parse(file, size, r.ps);
    if (pr != kParsed)
        return (int)pr;
    const Geom& g = r.ps.g;
    r.coef.assign((size_t)g.nblocks * 64 + 64, 0);  // (+64: nothing may be read there; a sanitizer would tell)
    r.coef.resize((size_t)g.nblocks * 64);
    std::vector<uint32_t> dd(g.nblocks);
    std::vector<uint64_t> ddoff((size_t)g.nblocks + 1);
    jp::ScanArgs a{};
    a.g = g, a.S = S, a.coef = r.coef.data(), a.dd = dd.data(), a.ddoff = ddoff.data();
    for (const jp::PScan& sc : r.ps.scans) {
        const std::vector<uint32_t> subfirst = jp::sub_first(sc, S);
        const uint32_t nsub = subfirst.back(), nu = sc.segoff.back();
        // unstuffing as the kernels do it: the scan with the marker behind it in zero-padded pieces
        const uint32_t scan_len = (uint32_t)sc.scan_len, pieces = (scan_len + kPiece - 1) / kPiece;
        std::vector<uint8_t> scan(((size_t)pieces + 1) * kPiece, 0);
        std::memcpy(scan.data(), file + sc.scan_start, (size_t)scan_len + 2);
        std::vector<uint64_t> dropoff(pieces + 1, 0);
        for (uint32_t p = 0; p < pieces; p++) {
            uint32_t prev = p ? scan[(size_t)p * kPiece - 1] : 0u, n = 0;
            for (int j = 0; j < kPiece; j++) {
                const size_t at = (size_t)p * kPiece + j;
                n += (at < scan_len && dropped(prev, scan[at], scan[at + 1])) ? 1u : 0u;
                prev = scan[at];
            }
            dropoff[p + 1] = dropoff[p] + n;
        }
        if (scan_len - dropoff[pieces] != nu)
            return -1;
        std::vector<uint32_t> u(nu / 4 + 3, 0);
        for (uint32_t p = 0; p < pieces; p++) {
            uint8_t* dst = (uint8_t*)u.data() + ((uint64_t)p * kPiece - dropoff[p]);
            uint32_t prev = p ? scan[(size_t)p * kPiece - 1] : 0u;
            for (int j = 0; j < kPiece; j++) {
                const size_t at = (size_t)p * kPiece + j;
                if (at < scan_len && !dropped(prev, scan[at], scan[at + 1]))
                    *dst++ = scan[at];
                prev = scan[at];
            }
        }
        // the rounds
        std::vector<jp::PState> ex[2] = {std::vector<jp::PState>(nsub), std::vector<jp::PState>(nsub)}, last(nsub);
        std::vector<uint32_t> count(nsub);
        std::vector<uint64_t> first((size_t)nsub + 1, 0);
        a.sc = sc.sc, a.tab = &sc.tab, a.u = u.data(), a.segoff = sc.segoff.data(), a.subfirst = subfirst.data(), a.nsub = nsub;
        a.exit[0] = ex[0].data(), a.exit[1] = ex[1].data(), a.last = last.data(), a.count = count.data(), a.first = first.data();
        const Table* t = &sc.tab.dc[0];  // dc[4] and ac[4] lie back to back, as in the kernels' LDS
        for (uint32_t i = 0; i < nsub; i++)
            jp::init_lane(a, i);
        uint32_t rd = 0;
        for (;;) {
            rd++;
            bool flag = false;
            for (uint32_t i = 0; i < nsub; i++)
                flag |= jp::sync_lane(a, i, rd, t);
            if (!flag || rd > nsub)
                break;
        }
        r.scan_rounds.push_back(rd), r.scan_nsub.push_back(nsub);
        // the block-count scan and the last pass
        for (uint32_t i = 0; i < nsub; i++)
            first[i + 1] = first[i] + count[i];
        uint32_t err = jp::kNoError;
        for (uint32_t i = 0; i < nsub; i++) {
            const jp::Sub s = jp::sub_of(a, i);
            r.entry.push_back(s.first ? jp::seg_entry(a.sc, s) : ex[rd & 1][i - 1]);
            r.count.push_back(count[i]);
            err = std::min(err, jp::write_lane(a, i, rd, t));
        }
        if (err != jp::kNoError) {
            r.err = err, r.err_scan = (uint32_t)(r.scan_rounds.size() - 1);
            return 3;
        }
        if (sc.sc.kind == jp::kDCFirst) {
            ddoff[0] = 0;
            for (uint32_t k = 0; k < sc.sc.nunits; k++)
                ddoff[k + 1] = ddoff[k] + dd[k];
            for (uint32_t k = 0; k < sc.sc.nunits; k++)
                jp::dcput_lane(a, k);
        }
        if (r.keep)
            r.after.push_back(r.coef);
    }
    return 0;
}

// the DC differences, then the sequential decoder's pixel stage (a copy of tests/host_jpegdec/jpegdec_emul.hip's)
void to_pixels(Run& r, int out_cn, uint8_t* out)
{
    const Geom& g = r.ps.g;
    const Tables& t = r.ps.tab;
    std::vector<uint32_t> dd(g.nblocks), dcd(g.nblocks);
    jp::ScanArgs a{};
    a.g = g, a.coef = r.coef.data(), a.dd = dd.data();
    for (uint32_t b = 0; b < g.nblocks; b++)
        jp::dcsave_lane(a, b);
    for (uint32_t b = 0; b < g.nblocks; b++)
        jp::dcdiff_lane(a, b);
    for (uint32_t b = 0; b < g.nblocks; b++) {
        uint32_t pos, pos0;
        dc_pos(g, b, pos, pos0);
        dcd[pos] = (uint32_t)(int)r.coef[(size_t)b * 64];
    }
    std::vector<uint64_t> dcoff((size_t)g.nblocks + 1, 0);
    for (uint32_t b = 0; b < g.nblocks; b++)
        dcoff[b + 1] = dcoff[b] + dcd[b];
    std::vector<uint8_t> plane[3];
    for (uint32_t c = 0; c < g.nc; c++)
        plane[c].assign((size_t)plane_pitch(g, c) * plane_rows(g, c), 0);
    for (uint32_t b = 0; b < g.nblocks; b++) {
        const BlockPos pos = block_pos(g, b);
        const uint16_t* q = t.q[g.tq[pos.comp]];
        int tile[8][8];
        for (int c = 0; c < 8; c++) {
            int d[8];
            for (int i = 0; i < 8; i++)
                d[i] = dequantise(r.coef[(size_t)b * 64 + zigzag_of(i * 8 + c)], q[i * 8 + c]);
            if (c == 0) {
                uint32_t at, at0;
                dc_pos(g, b, at, at0);
                d[0] = dequantise((int16_t)(uint32_t)(dcoff[at + 1] - dcoff[at0]), q[0]);
            }
            idct_pass<11>(d);
            for (int i = 0; i < 8; i++)
                tile[i][c] = d[i];
        }
        for (int row = 0; row < 8; row++) {
            int d[8];
            for (int c = 0; c < 8; c++)
                d[c] = tile[row][c];
            idct_pass<18>(d);
            for (int c = 0; c < 8; c++)
                plane[pos.comp][(size_t)(pos.y0 + row) * plane_pitch(g, pos.comp) + pos.x0 + c] = (uint8_t)clamp255(d[c] + 128);
        }
    }
    for (uint32_t y = 0; y < g.h; y++)
        for (uint32_t x = 0; x < g.w; x++) {
            uint8_t* px = out + ((size_t)y * g.w + x) * out_cn;
            const int lum = plane[0][(size_t)y * plane_pitch(g, 0) + x];
            if (g.nc == 1) {
                for (int k = 0; k < out_cn; k++)
                    px[k] = (uint8_t)lum;
            } else {
                ycc_to_bgr(lum, chroma_sample(plane[1].data(), plane_pitch(g, 1), g, x, y),
                           chroma_sample(plane[2].data(), plane_pitch(g, 1), g, x, y), px);
            }
        }
}

}  // namespace

extern "C" {

// info: height, width, components, h_samp, v_samp, scans, blocks, 0
int jprog_emul_info(const uint8_t* file, uint64_t size, int32_t* info)
{
    jp::PParsed p;
    const ParseResult r = jp::parse(file, size, p);
    if (r != kParsed)
        return (int)r;
    const int32_t v[8] = {(int32_t)p.g.h, (int32_t)p.g.w, (int32_t)p.g.nc, (int32_t)p.g.hs, (int32_t)p.g.vs, (int32_t)p.scans.size(),
                          (int32_t)p.g.nblocks, 0};
    std::memcpy(info, v, sizeof(v));
    return 0;
}

// after: scans x nblocks x 64, the store behind every scan (DC as values; at most scan_cap scans); states: 5 words per subsequence
// (p, z, c, run, b) and counts: one, of all scans back to back, at most sub_cap; scan_rounds, scan_nsub: per scan;
// report: scans, subsequences, rounds, error bit, error scan; pixels: h x w x out_cn, dense
int jprog_emul_decode(const uint8_t* file, uint64_t size, uint32_t S, int out_cn, int16_t* after, uint32_t scan_cap, uint32_t* states,
                      uint32_t* counts, uint32_t sub_cap, uint32_t* scan_rounds, uint32_t* scan_nsub, uint32_t* report, uint8_t* pixels)
{
    Run r;
    r.keep = true;
    const int rc = run(file, size, S ? S : kDefaultSubseqBits, r);
    if (rc != 0 && rc != 3)
        return rc;
    uint32_t rounds = 0;
    for (uint32_t v : r.scan_rounds)
        rounds += v;
    report[0] = (uint32_t)r.ps.scans.size(), report[1] = (uint32_t)r.entry.size(), report[2] = rounds, report[3] = r.err, report[4] = r.err_scan;
    if (rc == 3)
        return rc;
    if (r.entry.size() > sub_cap || r.ps.scans.size() > scan_cap)
        return -2;
    for (size_t s = 0; s < r.after.size(); s++) {
        std::memcpy(after + s * r.coef.size(), r.after[s].data(), r.coef.size() * 2);
        scan_rounds[s] = r.scan_rounds[s], scan_nsub[s] = r.scan_nsub[s];
    }
    for (size_t i = 0; i < r.entry.size(); i++) {
        const jp::PState& e = r.entry[i];
        states[5 * i] = e.p, states[5 * i + 1] = e.zc & 255u, states[5 * i + 2] = e.zc >> 8, states[5 * i + 3] = e.run, states[5 * i + 4] = e.b;
        counts[i] = r.count[i];
    }
    to_pixels(r, out_cn, pixels);
    return 0;
}

}

#ifdef JPROG_MAIN
// decodes every file named on the command line at two subsequence sizes and prints one line per file; the exit status is 0 unless a
// file cannot be read or the decomposition disagrees with the parse
int main(int argc, char** argv)
{
    int bad = 0;
    for (int i = 1; i < argc; i++) {
        std::FILE* f = std::fopen(argv[i], "rb");
        if (!f) {
            bad = 1;
            continue;
        }
        std::vector<uint8_t> data;
        uint8_t buf[4096];
        for (size_t n; (n = std::fread(buf, 1, sizeof(buf), f)) > 0;)
            data.insert(data.end(), buf, buf + n);
        std::fclose(f);
        // (an exact-size heap copy: a read one byte past the file is a sanitizer report)
        std::vector<uint8_t> exact(data.begin(), data.end());
        exact.shrink_to_fit();
        for (uint32_t S : {256u, 1024u}) {
            Run r;
            const int rc = run(exact.data(), exact.size(), S, r);
            unsigned long sum = 0;
            uint32_t rounds = 0;
            for (uint32_t v : r.scan_rounds)
                rounds += v;
            if (rc == 0) {
                std::vector<uint8_t> px((size_t)r.ps.g.h * r.ps.g.w * 3);
                to_pixels(r, 3, px.data());
                for (uint8_t v : px)
                    sum += v;
            }
            std::printf("%s S=%u rc=%d rounds=%u sum=%lu\n", argv[i], S, rc, rounds, sum);
            if (rc < 0)
                bad = 1;
        }
    }
    return bad;
}
#endif
