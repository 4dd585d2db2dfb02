// jpegdec_emul.hip -- TEST HARNESS: runs the product's JPEG decoding arithmetic (jpegdec_core.hpp: the step function, F_i, the last pass,
// the inverse DCT, upsampling and colour) and its host side (jpegdec_host.hpp: the parse, the tables, the segments) on the CPU, in a
// sequential copy of the kernels' decomposition: drop counts per 16-byte piece, their scan, the placement; rounds over all
// subsequences with two exit buffers, the skip rule and the flag; the block-count scan; the last pass; the DC scan by component and
// its subtraction; blocks to planes; planes to pixels.
//
// Built by tests/test_jpegdec_host.py itself (hipcc --cuda-host-only -O2 -shared -fPIC, into a temporary directory) and compared there
// with the restatement (tests/jpgdec_ref.py).  With -DJDEC_MAIN it is a stand-alone program that decodes the files named on its
// command line -- the form the sanitizer run takes.  Not part of the product: nothing in vr180_convert_amd/ loads it.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/vr180_remap.h"
#include "../../vr180_convert_amd/csrc/jpegdec_host.hpp"

using namespace v1c::jpegdec;

namespace {

struct Run {
    Parsed ps;
    std::vector<uint32_t> subfirst, u, count;
    std::vector<State> entry;
    std::vector<int16_t> coef;
    uint32_t rounds = 0, err = 0xffffffffu;
};

struct SubE {
    uint32_t k, start, end, E;
    bool first, last;
};

SubE sub_of(const Run& r, uint32_t i, uint32_t S)
{
    uint32_t lo = 0, hi = r.ps.g.nseg - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (r.subfirst[mid] <= i)
            lo = mid;
        else
            hi = mid - 1;
    }
    SubE s;
    s.k = lo, s.E = 8 * r.ps.segoff[lo + 1];
    const uint32_t j = i - r.subfirst[lo];
    s.start = 8 * r.ps.segoff[lo] + j * S;
    s.end = std::min(s.start + S, s.E);
    s.first = j == 0, s.last = i + 1 == r.subfirst[lo + 1];
    return s;
}

// 0: decoded, 1: unsupported, 2: corrupt by the parse, 3: corrupt by the last pass, -1: the decomposition disagrees with the parse
int run(const uint8_t* file, uint64_t size, uint32_t S, Run& r)
{
    const ParseResult pr = parse(file, size, r.ps);
    if (pr != kParsed)
        return (int)pr;
    const Geom& g = r.ps.g;
    r.subfirst = sub_first(r.ps, S);
    const uint32_t nsub = r.subfirst.back(), nu = r.ps.segoff.back();
    // unstuffing as the kernels do it: the scan with the marker behind it in zero-padded pieces
    const uint32_t scan_len = (uint32_t)r.ps.scan_len, pieces = (scan_len + kPiece - 1) / kPiece;
    std::vector<uint8_t> scan(((size_t)pieces + 1) * kPiece, 0);
    std::memcpy(scan.data(), file + r.ps.scan_start, (size_t)scan_len + 2);
    std::vector<uint32_t> drop(pieces);
    for (uint32_t p = 0; p < pieces; p++) {
        uint32_t prev = p ? scan[(size_t)p * kPiece - 1] : 0u, n = 0;
        for (int j = 0; j < kPiece; j++) {
            const size_t at = (size_t)p * kPiece + j;
            n += (at < scan_len && dropped(prev, scan[at], scan[at + 1])) ? 1u : 0u;
            prev = scan[at];
        }
        drop[p] = n;
    }
    std::vector<uint64_t> dropoff(pieces + 1, 0);
    for (uint32_t p = 0; p < pieces; p++)
        dropoff[p + 1] = dropoff[p] + drop[p];
    if (scan_len - dropoff[pieces] != nu)
        return -1;
    r.u.assign(nu / 4 + 3, 0);
    for (uint32_t p = 0; p < pieces; p++) {
        uint8_t* dst = (uint8_t*)r.u.data() + ((uint64_t)p * kPiece - dropoff[p]);
        uint32_t prev = p ? scan[(size_t)p * kPiece - 1] : 0u;
        for (int j = 0; j < kPiece; j++) {
            const size_t at = (size_t)p * kPiece + j;
            if (at < scan_len && !dropped(prev, scan[at], scan[at + 1]))
                *dst++ = scan[at];
            prev = scan[at];
        }
    }
    // the rounds
    const TablePair tp = table_pair(g, r.ps.tab.dc, r.ps.tab.ac);
    std::vector<State> ex[2] = {std::vector<State>(nsub), std::vector<State>(nsub)}, last(nsub, State{0xffffffffu, 0xffffffffu});
    r.count.assign(nsub, 0);
    for (uint32_t i = 0; i < nsub; i++)
        ex[0][i] = State{sub_of(r, i, S).end, 0u};
    uint32_t rd = 0;
    for (;;) {
        rd++;
        const std::vector<State>& in = ex[(rd - 1) & 1];
        std::vector<State>& out = ex[rd & 1];
        bool flag = false;
        for (uint32_t i = 0; i < nsub; i++) {
            const SubE s = sub_of(r, i, S);
            const State e = s.first ? State{s.start, 0u} : in[i - 1];
            if (e == last[i]) {
                out[i] = in[i];
                continue;
            }
            State x = e;
            r.count[i] = decode_span<false>(r.u.data(), tp, g.bpm, x, s.end, s.E, nullptr, 0, 0, nullptr);
            last[i] = e, out[i] = x;
            flag |= !s.last && !(x == in[i]);
        }
        if (!flag || rd > nsub)
            break;
    }
    r.rounds = rd;
    r.entry.resize(nsub);
    // the block-count scan and the last pass
    std::vector<uint64_t> first(nsub + 1, 0);
    for (uint32_t i = 0; i < nsub; i++)
        first[i + 1] = first[i] + r.count[i];
    r.coef.assign((size_t)g.nblocks * 64, 0);
    for (uint32_t i = 0; i < nsub; i++) {
        const SubE s = sub_of(r, i, S);
        State e = s.first ? State{s.start, 0u} : ex[rd & 1][i - 1];
        r.entry[i] = e;
        const uint32_t i0 = r.subfirst[s.k], b0 = s.k * g.ibl, bq = std::min(b0 + g.ibl, g.nblocks);
        const uint64_t done = first[i] - first[i0];
        const uint32_t b = done < bq - b0 ? b0 + (uint32_t)done : bq;
        uint32_t err = 0xffffffffu;
        decode_span<true>(r.u.data(), tp, g.bpm, e, s.end, s.E, r.coef.data(), b, bq, &err);
        if (s.first && first[r.subfirst[s.k + 1]] - first[i0] != bq - b0)
            err = std::min(err, s.start);
        r.err = std::min(r.err, err);
    }
    return r.err == 0xffffffffu ? 0 : 3;
}

void to_pixels(const Run& r, int out_cn, uint8_t* out)
{
    const Geom& g = r.ps.g;
    const Tables& t = r.ps.tab;
    // the DC scan: differences by component, the exclusive sums modulo 2^32, the subtraction at the segment's start
    std::vector<uint32_t> dcd(g.nblocks);
    for (uint32_t b = 0; b < g.nblocks; b++) {
        uint32_t pos, pos0;
        dc_pos(g, b, pos, pos0);
        dcd[pos] = (uint32_t)(int)r.coef[(size_t)b * 64];
    }
    std::vector<uint64_t> dcoff(g.nblocks + 1, 0);
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

// info: height, width, components, h_samp, v_samp, restart interval, segments, blocks
int jdec_emul_info(const uint8_t* file, uint64_t size, int32_t* info)
{
    Parsed p;
    const ParseResult r = parse(file, size, p);
    if (r != kParsed)
        return (int)r;
    const int32_t v[8] = {(int32_t)p.g.h, (int32_t)p.g.w, (int32_t)p.g.nc, (int32_t)p.g.hs, (int32_t)p.g.vs, (int32_t)p.restart,
                          (int32_t)p.g.nseg, (int32_t)p.g.nblocks};
    std::memcpy(info, v, sizeof(v));
    return 0;
}

// coef: nblocks x 64 (the DC a difference); states: 3 words per subsequence (p, z, c) and counts: one, both of `cap` subsequences;
// report: segments, subsequences, rounds, error bit; pixels: h x w x out_cn, dense
int jdec_emul_decode(const uint8_t* file, uint64_t size, uint32_t S, int out_cn, int16_t* coef, uint32_t* states, uint32_t* counts, uint32_t cap,
                     uint32_t* report, uint8_t* pixels)
{
    Run r;
    const int rc = run(file, size, S ? S : kDefaultSubseqBits, r);
    if (rc != 0 && rc != 3)
        return rc;
    const uint32_t nsub = r.subfirst.back();
    report[0] = r.ps.g.nseg, report[1] = nsub, report[2] = r.rounds, report[3] = r.err;
    if (rc == 3)
        return rc;
    if (nsub > cap)
        return -2;
    std::memcpy(coef, r.coef.data(), r.coef.size() * 2);
    for (uint32_t i = 0; i < nsub; i++) {
        states[3 * i] = r.entry[i].p, states[3 * i + 1] = r.entry[i].zc & 255u, states[3 * i + 2] = r.entry[i].zc >> 8;
        counts[i] = r.count[i];
    }
    to_pixels(r, out_cn, pixels);
    return 0;
}

}

#ifdef JDEC_MAIN
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
            if (rc == 0) {
                std::vector<uint8_t> px((size_t)r.ps.g.h * r.ps.g.w * 3);
                to_pixels(r, 3, px.data());
                for (uint8_t v : px)
                    sum += v;
            }
            std::printf("%s S=%u rc=%d rounds=%u sum=%lu\n", argv[i], S, rc, r.rounds, sum);
            if (rc < 0)
                bad = 1;
        }
    }
    return bad;
}
#endif
