// feat_emul.hip -- TEST HARNESS: runs the product's feature arithmetic (feat_core.hpp) on the CPU, image by image and keypoint by keypoint.
//
// Built by tests/test_feat_host.py itself (hipcc --cuda-host-only -O2 -shared -fPIC, into a temporary directory) and compared there with
// the NumPy restatement of the contract (tests/feat_ref.py).  Not part of the product: nothing in vr180_convert_amd/ loads it.
#include <algorithm>

#include "../../vr180_convert_amd/csrc/feat_core.hpp"

using namespace v1c::feat;

extern "C" {

void feat_resample(const uint8_t* img, int h, int w, int64_t pitch, int cn, const int32_t* rb, const int32_t* cb, int wh, int ww,
                   uint8_t* out)
{
    (void)h;
    (void)w;
    for (int y = 0; y < wh; y++)
        for (int x = 0; x < ww; x++) {
            int sum = 0;
            for (int r = rb[y]; r < rb[y + 1]; r++)
                for (int c = cb[x]; c < cb[x + 1]; c++)
                    sum += luma(img + (int64_t)r * pitch + (int64_t)c * cn, cn);
            out[(int64_t)y * ww + x] = (uint8_t)block_mean(sum, (rb[y + 1] - rb[y]) * (cb[x + 1] - cb[x]));
        }
}

void feat_smooth(const uint8_t* in, int h, int w, uint8_t* out)
{
    auto px = [&](int y, int x) { return (int)in[(int64_t)std::min(std::max(y, 0), h - 1) * w + std::min(std::max(x, 0), w - 1)]; };
    auto hor = [&](int y, int x) { return smooth5(px(y, x - 2), px(y, x - 1), px(y, x), px(y, x + 1), px(y, x + 2)); };
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            out[(int64_t)y * w + x] = (uint8_t)smooth5(hor(y - 2, x), hor(y - 1, x), hor(y, x), hor(y + 1, x), hor(y + 2, x));
}

void feat_fast(const uint8_t* y, int h, int w, int32_t* out)
{
    for (int j = 0; j < h; j++)
        for (int i = 0; i < w; i++)
            out[(int64_t)j * w + i] = (j >= 3 && j < h - 3 && i >= 3 && i < w - 3) ? fast_score(y, w, i, j) : -256;
}

void feat_nms(const uint8_t* s, int h, int w, uint8_t* keep)
{
    for (int j = 0; j < h; j++)
        for (int i = 0; i < w; i++)
            keep[(int64_t)j * w + i] = j >= 1 && j < h - 1 && i >= 1 && i < w - 1 && s[(int64_t)j * w + i] && nms_keep(s, w, i, j);
}

// per keypoint: m10, m01 and the sector
void feat_orient(const uint8_t* sm, int w, const int32_t* xy, int n, const int32_t* bv, int32_t* out)
{
    for (int k = 0; k < n; k++) {
        const uint8_t* c = sm + (int64_t)xy[2 * k + 1] * w + xy[2 * k];
        int m10 = 0, m01 = 0;
        for (int q = 0; q < (2 * kPatchRadius + 1) * (2 * kPatchRadius + 1); q++) {
            int dx, dy;
            if (disc_offset(q, &dx, &dy)) {
                m10 += dx * c[(int64_t)dy * w + dx];
                m01 += dy * c[(int64_t)dy * w + dx];
            }
        }
        out[3 * k] = m10;
        out[3 * k + 1] = m01;
        out[3 * k + 2] = orient_bin(m10, m01, bv);
    }
}

// per query: (d1, idx, d2) over candidates split into chunks of `chunk` merged in order, as the kernels do
void feat_best(const uint8_t* q, int nq, const uint8_t* t, int nt, int chunk, int32_t* out)
{
    for (int i = 0; i < nq; i++) {
        Best acc = best_init();
        for (int j0 = 0; j0 < nt; j0 += chunk) {
            Best b = best_init();
            for (int j = j0; j < std::min(nt, j0 + chunk); j++)
                best_push(b, hamming256((const uint32_t*)(q + (int64_t)i * 32), (const uint32_t*)(t + (int64_t)j * 32)), j);
            acc = j0 == 0 ? b : best_merge(acc, b);
        }
        out[3 * i] = acc.d1;
        out[3 * i + 1] = acc.idx;
        out[3 * i + 2] = acc.d2;
    }
}

}  // extern "C"
