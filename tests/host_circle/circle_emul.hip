// circle_emul.hip -- host build of the image-circle fit: circle_core.hpp as the kernels compile it, driven through the kernels'
// decomposition (kernels_circle.hip) -- rows in steps of 64 pixels with the ballot as a loop over the lanes, columns as one record per
// band of 64 rows and a walk down and up through the records, the fit's sums as 512 strided partial sums that are then added up.  Built as a shared library for
// tests/test_circle_host.py and, with -DCIRCLE_MAIN, as a program of its own that the sanitizers run over the cases.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../vr180_convert_amd/csrc/circle_core.hpp"

using namespace v1c::circle;

namespace {

constexpr int kFitThreads = 512;

struct Image {
    const uint8_t* p;
    int h, w;
    int64_t pitch;
    int cn;
    bool depth16;
    int sum(int y, int x) const
    {
        const uint8_t* q = p + (int64_t)y * pitch;
        int s = 0;
        for (int c = 0; c < cn; c++) {
            if (depth16) {
                uint16_t v;
                std::memcpy(&v, q + ((int64_t)x * cn + c) * 2, 2);
                s += v;
            } else {
                s += q[(int64_t)x * cn + c];
            }
        }
        return s;
    }
};

int scan_row(const Image& im, int y, bool rev, int thr_cn, int run)
{
    uint64_t pm = 0;
    for (int d0 = 0; d0 < im.w; d0 += 64) {
        uint64_t m = 0;
        for (int lane = 0; lane < 64; lane++) {
            const int d = d0 + lane;
            if (d < im.w && im.sum(y, rev ? im.w - 1 - d : d) >= thr_cn)
                m |= 1ull << lane;
        }
        const uint64_t t = run_ends(m, pm, run);
        if (t)
            return d0 + ctz64(t) - run + 1;
        pm = m;
    }
    return -1;
}

}  // namespace

// prm: threshold, run, rounds, min_points, tol16[8].  points: capacity 2 (h + w) records (x, y, selected).  Returns the point count.
extern "C" int circle_emul_fit(const void* img, int h, int w, int64_t pitch, int cn, int depth16, const int32_t* prm, double* out,
                               int32_t* points)
{
    Params p;
    p.threshold = prm[0];
    p.run = prm[1];
    p.rounds = prm[2];
    p.min_points = prm[3];
    for (int k = 0; k < kMaxRounds; k++)
        p.tol16[k] = prm[4 + k];
    const Image im{(const uint8_t*)img, h, w, pitch, cn, depth16 != 0};
    const int thr_cn = p.threshold * cn;
    const size_t n = 2 * ((size_t)h + w);
    std::vector<uint32_t> pts(n, kNoPoint);
    std::vector<uint8_t> sel(n, 0);
    for (int y = 0; y < h; y++) {
        const int xl = scan_row(im, y, false, thr_cn, p.run);
        int xr = -1;
        if (xl >= 0)
            xr = w - 1 - scan_row(im, y, true, thr_cn, p.run);
        pts[2 * y] = xl > 0 && xl < w - 1 ? pack_point(xl, y) : kNoPoint;
        pts[2 * y + 1] = xr > 0 && xr < w - 1 ? pack_point(xr, y) : kNoPoint;
    }
    // k_circle_col_bands: one record per band and column; k_circle_col_join: down and up through them
    const int nb = (h + kBandRows - 1) / kBandRows;
    std::vector<uint32_t> rec((size_t)nb * w);
    for (int b = 0; b < nb; b++)
        for (int x = 0; x < w; x++) {
            const int y0b = b * kBandRows, rows = h - y0b < kBandRows ? h - y0b : kBandRows;
            BandScan bs;
            for (int o = 0; o < rows; o++)
                band_step(bs, im.sum(y0b + o, x) >= thr_cn, o, p.run);
            rec[(size_t)b * w + x] = band_pack(bs, rows);
        }
    for (int x = 0; x < w; x++) {
        ColJoin down, up;
        for (int b = 0; b < nb; b++) {
            const int bu = nb - 1 - b;
            join_step(down, rec[(size_t)b * w + x], b * kBandRows, h - b * kBandRows < kBandRows ? h - b * kBandRows : kBandRows, p.run, true);
            join_step(up, rec[(size_t)bu * w + x], bu * kBandRows, h - bu * kBandRows < kBandRows ? h - bu * kBandRows : kBandRows, p.run, false);
        }
        const int yt = down.found, yb = up.found;
        pts[2 * (size_t)h + 2 * x] = yt > 0 && yt < h - 1 ? pack_point(x, yt) : kNoPoint;
        pts[2 * (size_t)h + 2 * x + 1] = yb > 0 && yb < h - 1 ? pack_point(x, yb) : kNoPoint;
    }
    // k_circle_fit
    const int x0 = w / 2, y0 = h / 2;
    int64_t cx16 = 0, cy16 = 0, r16 = 0, n_rim = 0, n_used = 0;
    Fit f{0.0, 0.0, 0.0, 0};
    int status = 0;
    for (int round = -1; round < p.rounds; round++) {
        const int64_t t16 = round >= 0 ? p.tol16[round] : 0;
        std::vector<int64_t> part((size_t)kFitThreads * kSums, 0);
        for (int tid = 0; tid < kFitThreads; tid++) {
            int64_t* a = &part[(size_t)tid * kSums];
            for (size_t i = tid; i < n; i += kFitThreads) {
                const uint32_t q = pts[i];
                bool in = q != kNoPoint;
                const int x = (int)(q & 0xFFFFu) - x0, y = (int)(q >> 16) - y0;
                if (in && round >= 0)
                    in = selected(dist2_16(x, y, cx16, cy16), r16, t16);
                sel[i] = in ? 1 : 0;
                if (in) {
                    const int xx = x * x, yy = y * y, z = xx + yy;
                    a[0] += 1;
                    a[1] += x;
                    a[2] += y;
                    a[3] += xx;
                    a[4] += (int64_t)x * y;
                    a[5] += yy;
                    a[6] += (int64_t)x * z;
                    a[7] += (int64_t)y * z;
                    a[8] += z;
                }
            }
        }
        int64_t a[kSums] = {0};
        for (int tid = 0; tid < kFitThreads; tid++)
            for (int k = 0; k < kSums; k++)
                a[k] += part[(size_t)tid * kSums + k];
        if (round < 0)
            n_rim = a[0];
        n_used = a[0];
        f = a[0] < p.min_points ? Fit{0.0, 0.0, 0.0, 1} : solve(a, h, w);
        status = f.status;
        cx16 = q16(f.cx);
        cy16 = q16(f.cy);
        r16 = q16(f.r);
        if (status)
            break;
    }
    int64_t e = 0;
    if (!status)
        for (size_t i = 0; i < n; i++)
            if (sel[i]) {
                const int64_t d = isqrt64(dist2_16((int)(pts[i] & 0xFFFFu) - x0, (int)(pts[i] >> 16) - y0, cx16, cy16)) - r16;
                e += d * d;
            }
    out[0] = status ? 0.0 : (double)x0 + f.cx;
    out[1] = status ? 0.0 : (double)y0 + f.cy;
    out[2] = status ? 0.0 : f.r;
    out[3] = (double)status;
    out[4] = (double)n_rim;
    out[5] = (double)n_used;
    out[6] = status ? 0.0 : rms16(e, n_used);
    out[7] = 0.0;
    int m = 0;
    for (size_t i = 0; i < n; i++)
        if (pts[i] != kNoPoint) {
            points[3 * m] = (int32_t)(pts[i] & 0xFFFFu);
            points[3 * m + 1] = (int32_t)(pts[i] >> 16);
            points[3 * m + 2] = sel[i];
            m++;
        }
    return m;
}

#ifdef CIRCLE_MAIN
// circle_san LIST: every line of LIST is "h w pitch cn depth16 offset threshold run rounds min_points t0 .. t7 file"; the image is a
// heap copy of the file's exact size, read from byte `offset`.  Prints the eight doubles (hex floats) and the points of every case.
int main(int argc, char** argv)
{
    if (argc != 2)
        return 2;
    FILE* list = std::fopen(argv[1], "r");
    if (!list)
        return 2;
    int h, w, cn, d16;
    long long pitch, offset;
    int32_t prm[12];
    char path[4096];
    while (std::fscanf(list, "%d %d %lld %d %d %lld %d %d %d %d %d %d %d %d %d %d %d %d %4095s", &h, &w, &pitch, &cn, &d16, &offset, &prm[0], &prm[1],
                       &prm[2], &prm[3], &prm[4], &prm[5], &prm[6], &prm[7], &prm[8], &prm[9], &prm[10], &prm[11], path) == 19) {
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
        std::vector<int32_t> points(6 * ((size_t)h + w));
        double out[8];
        const int m = circle_emul_fit(buf + offset, h, w, pitch, cn, d16, prm, out, points.data());
        for (int k = 0; k < 8; k++)
            std::printf("%a ", out[k]);
        std::printf("%d", m);
        for (int k = 0; k < 3 * m; k++)
            std::printf(" %d", points[k]);
        std::printf("\n");
        std::free(buf);
    }
    std::fclose(list);
    return 0;
}
#endif
