// colormatch_emul.hip -- host build of the colour match: colormatch_core.hpp as the kernels compile it, driven through the kernels'
// decomposition (kernels_colormatch.hip) -- the rows as items of a grid of `blocks` x 256 threads, every thread with its six run slots,
// every wave with its own copy of the histograms, the copies of a workgroup summed and added to the workspace; the tables by 256
// threads with the ballot as a loop over the lanes and the scan step by step; the apply over the same items.  Built as a shared library
// for tests/test_colormatch_host.py and, with -DCOLORMATCH_MAIN, as a program of its own that the sanitizers run over the cases.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../vr180_convert_amd/csrc/colormatch_core.hpp"

using namespace v1c::colormatch;

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

struct WaveAdd {
    uint32_t* mine;
    void operator()(int slot, int bin, uint32_t count) const { mine[slot * kBins + bin] += count; }
};

template <int CN>
void hist(const uint8_t* left, int64_t pitch_l, const uint8_t* right, int64_t pitch_r, int h, int w, int lo, int hi, int blocks, uint32_t* out)
{
    constexpr int CC = CN == 1 ? 1 : 3;
    const int per_row = segs_of(w) + 1;
    const int64_t items = (int64_t)h * per_row;
    for (int blk = 0; blk < blocks; blk++) {
        std::vector<uint32_t> copies((size_t)kWaves * kHistWords, 0);
        for (int tid = 0; tid < kThreads; tid++) {
            WaveAdd add{copies.data() + (size_t)(tid >> 6) * kHistWords};
            RunSlot rs[6];
            for (int64_t it = (int64_t)blk * kThreads + tid; it < items; it += (int64_t)blocks * kThreads) {
                const int y = (int)(it / per_row), s = (int)(it - (int64_t)y * per_row);
                const uint8_t* rl = left + (int64_t)y * pitch_l;
                const uint8_t* rr = right + (int64_t)y * pitch_r;
                const int x0 = head_of((unsigned)((uintptr_t)rl & 15u), CN, w);
                const int nseg = (w - x0) / kSegPixels;
                const int x1 = x0 + nseg * kSegPixels;
                int xa, xb;  // this item's pixels: a segment, or the head and the tail
                if (s < per_row - 1) {
                    if (s >= nseg)
                        continue;
                    xa = x0 + s * kSegPixels;
                    xb = xa + kSegPixels;
                } else {
                    xa = 0;
                    xb = w;
                }
                for (int x = xa; x < xb; x++) {
                    if (s == per_row - 1 && x >= x0 && x < x1)
                        continue;
                    int l[3], r[3];
                    for (int c = 0; c < CC; c++) {
                        l[c] = rl[(int64_t)x * CN + c];
                        r[c] = rr[(int64_t)x * CN + c];
                    }
                    count_pixel<CC>(l, r, lo, hi, rs, add);
                }
            }
            run_flush(rs, add);
        }
        for (int i = 0; i < kHistWords; i++) {
            uint32_t t = 0;
            for (int v = 0; v < kWaves; v++)
                t += copies[(size_t)v * kHistWords + i];
            out[i] += t;
        }
    }
}

void build_luts(const uint32_t* hist_in, int cc, const Params& prm, uint8_t* luts, int32_t* report)
{
    static uint32_t cum[2][3][kBins];
    uint64_t pop[2][3][kWaves] = {}, knots[3][kWaves];
    int64_t wsum[2][3][kWaves] = {};
    for (int e = 0; e < 2; e++)
        for (int c = 0; c < 3; c++)
            for (int v = 0; v < kBins; v++) {
                const uint32_t t = hist_in[(e * 3 + c) * kBins + v];
                cum[e][c][v] = t;
                if (t)
                    pop[e][c][v >> 6] |= 1ull << (v & 63);
                wsum[e][c][v >> 6] += (int64_t)v * t;
            }
    const int ref = prm.reference, tgt = 1 - ref;
    for (int c = 0; c < 3; c++)
        for (int k = 0; k < kWaves; k++)
            knots[c][k] = pop[tgt][c][k] | (k == 0 ? 1ull : 0ull) | (k == kWaves - 1 ? 1ull << 63 : 0ull);
    for (int o = 1; o < kBins; o <<= 1)
        for (int k = 0; k < 6; k++) {
            uint32_t t[kBins];
            for (int v = 0; v < kBins; v++)
                t[v] = v >= o ? (&cum[0][0][0])[k * kBins + v - o] : 0;
            for (int v = 0; v < kBins; v++)
                (&cum[0][0][0])[k * kBins + v] += t[v];
        }
    const int64_t n = cum[0][0][kBins - 1];
    int64_t g[3] = {0, 0, 0};
    int status = n < prm.min_pixels ? 1 : 0;
    for (int c = 0; c < cc; c++)
        if (prm.mode == kModeGain) {
            int64_t sT = 0, sR = 0;
            for (int k = 0; k < kWaves; k++) {
                sT += wsum[tgt][c][k];
                sR += wsum[ref][c][k];
            }
            if (sT == 0)
                status = status ? status : 2;
            else
                g[c] = gain_of(sT, sR);
        }
    for (int c = 0; c < 3; c++)
        for (int v = 0; v < kBins; v++) {
            uint8_t m = (uint8_t)v;
            if (c < cc && status == 0)
                m = prm.mode == kModeGain ? gain_entry(v, g[c]) : histogram_entry(cum[tgt][c], cum[ref][c], knots[c], v, prm.max_shift);
            luts[c * kBins + v] = m;
        }
    for (int v = 0; v < kReportWords; v++) {
        int32_t r = 0;
        if (v == 0)
            r = status;
        else if (v == 1)
            r = (int32_t)n;
        else if (v < 17) {
            const int c = (v - 2) / 5, k = (v - 2) % 5;
            if (k == 4) {
                r = (int32_t)g[c];
            } else {
                const uint64_t* m = pop[k >> 1][c];
                r = -1;
                if (c < cc && (m[0] | m[1] | m[2] | m[3])) {
                    int q = (k & 1) ? kWaves - 1 : 0;
                    while (!m[q])
                        q += (k & 1) ? -1 : 1;
                    r = 64 * q + ((k & 1) ? high_bit64(m[q]) : low_bit64(m[q]));
                }
            }
        }
        report[v] = r;
    }
}

template <int CN>
void apply(const uint8_t* src, int64_t pitch_s, uint8_t* dst, int64_t pitch_d, int h, int w, const uint8_t* lut, int blocks)
{
    constexpr int CC = CN == 1 ? 1 : 3;
    const int per_row = segs_of(w) + 1;
    const int64_t items = (int64_t)h * per_row;
    for (int64_t t = 0; t < (int64_t)blocks * kThreads; t++)
        for (int64_t it = t; it < items; it += (int64_t)blocks * kThreads) {
            const int y = (int)(it / per_row), s = (int)(it - (int64_t)y * per_row);
            const uint8_t* rs = src + (int64_t)y * pitch_s;
            uint8_t* rd = dst + (int64_t)y * pitch_d;
            const int x0 = head_of((unsigned)((uintptr_t)rd & 15u), CN, w);
            const int nseg = (w - x0) / kSegPixels;
            const int x1 = x0 + nseg * kSegPixels;
            if (s < per_row - 1) {
                if (s >= nseg)
                    continue;
                uint8_t a[kSegPixels * CN];  // the segment read whole, then written whole, as the kernel's registers
                std::memcpy(a, rs + (int64_t)(x0 + s * kSegPixels) * CN, sizeof(a));
                for (int j = 0; j < kSegPixels * CN; j++)
                    a[j] = j % CN < CC ? lut[(j % CN) * kBins + a[j]] : a[j];
                std::memcpy(rd + (int64_t)(x0 + s * kSegPixels) * CN, a, sizeof(a));
            } else {
                for (int x = 0; x < w; x++) {
                    if (x >= x0 && x < x1)
                        continue;
                    for (int c = 0; c < CN; c++) {
                        const uint8_t val = rs[(int64_t)x * CN + c];
                        rd[(int64_t)x * CN + c] = c < CC ? lut[c * kBins + val] : val;
                    }
                }
            }
        }
}

}  // namespace

// prm: mode, reference, lo, hi, max_shift, min_pixels.  hist_out: 1536 uint32, luts: 768 bytes, report: 20 int32.
extern "C" void colormatch_emul_luts(const void* left, int64_t pitch_l, const void* right, int64_t pitch_r, int h, int w, int cn,
                                     const int32_t* prm, int blocks, uint32_t* hist_out, uint8_t* luts, int32_t* report)
{
    const Params p{prm[0], prm[1], prm[2], prm[3], prm[4], prm[5]};
    std::memset(hist_out, 0, kHistWords * sizeof(uint32_t));
    const uint8_t *l = (const uint8_t*)left, *r = (const uint8_t*)right;
    if (cn == 1)
        hist<1>(l, pitch_l, r, pitch_r, h, w, p.lo, p.hi, blocks, hist_out);
    else if (cn == 3)
        hist<3>(l, pitch_l, r, pitch_r, h, w, p.lo, p.hi, blocks, hist_out);
    else
        hist<4>(l, pitch_l, r, pitch_r, h, w, p.lo, p.hi, blocks, hist_out);
    build_luts(hist_out, cn == 1 ? 1 : 3, p, luts, report);
}

extern "C" void colormatch_emul_apply(const void* src, int64_t pitch_s, void* dst, int64_t pitch_d, int h, int w, int cn, const uint8_t* luts,
                                      int blocks)
{
    if (cn == 1)
        apply<1>((const uint8_t*)src, pitch_s, (uint8_t*)dst, pitch_d, h, w, luts, blocks);
    else if (cn == 3)
        apply<3>((const uint8_t*)src, pitch_s, (uint8_t*)dst, pitch_d, h, w, luts, blocks);
    else
        apply<4>((const uint8_t*)src, pitch_s, (uint8_t*)dst, pitch_d, h, w, luts, blocks);
}

#ifdef COLORMATCH_MAIN
// colormatch_san LIST: every line of LIST is "h w cn pitch_l offset_l pitch_r offset_r mode reference lo hi max_shift min_pixels blocks
// inplace file": both eyes are views into ONE heap copy of the file's exact size.  inplace 1: the target eye is rewritten where it is;
// 0: into a buffer of h * w * cn bytes.  Prints the histograms, the tables, the report and the result's bytes (hex) of every case.
int main(int argc, char** argv)
{
    if (argc != 2)
        return 2;
    FILE* list = std::fopen(argv[1], "r");
    if (!list)
        return 2;
    int h, w, cn, blocks, inplace;
    long long pl, ol, pr, orr;
    int32_t prm[6];
    char path[4096];
    while (std::fscanf(list, "%d %d %d %lld %lld %lld %lld %d %d %d %d %d %d %d %d %4095s", &h, &w, &cn, &pl, &ol, &pr, &orr, &prm[0], &prm[1],
                       &prm[2], &prm[3], &prm[4], &prm[5], &blocks, &inplace, path) == 16) {
        FILE* fp = std::fopen(path, "rb");
        if (!fp)
            return 3;
        std::fseek(fp, 0, SEEK_END);
        const long size = std::ftell(fp);
        std::fseek(fp, 0, SEEK_SET);
        uint8_t* buf = (uint8_t*)std::malloc(size > 0 ? size : 1);
        if (std::fread(buf, 1, size, fp) != (size_t)size)
            return 3;
        std::fclose(fp);
        std::vector<uint32_t> hs(kHistWords);
        uint8_t luts[kLutBytes];
        int32_t report[kReportWords];
        colormatch_emul_luts(buf + ol, pl, buf + orr, pr, h, w, cn, prm, blocks, hs.data(), luts, report);
        uint8_t* tgt = buf + (prm[1] == 0 ? orr : ol);
        const int64_t pt = prm[1] == 0 ? pr : pl;
        const size_t row = (size_t)w * cn;
        uint8_t* dst = inplace ? tgt : (uint8_t*)std::malloc((size_t)h * row);
        const int64_t pd = inplace ? pt : (int64_t)row;
        colormatch_emul_apply(tgt, pt, dst, pd, h, w, cn, luts, blocks);
        for (int i = 0; i < kHistWords; i++)
            std::printf("%u ", hs[i]);
        for (int i = 0; i < kLutBytes; i++)
            std::printf("%d ", luts[i]);
        for (int i = 0; i < kReportWords; i++)
            std::printf("%d ", report[i]);
        for (int y = 0; y < h; y++)
            for (size_t x = 0; x < row; x++)
                std::printf("%02x", dst[(int64_t)y * pd + x]);
        std::printf("\n");
        if (!inplace)
            std::free(dst);
        std::free(buf);
    }
    std::fclose(list);
    return 0;
}
#endif
