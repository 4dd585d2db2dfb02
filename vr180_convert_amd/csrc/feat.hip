// feat.hip -- host side of the feature-matching entry points of the C ABI (v1c_feat_*, include/vr180_remap.h): argument checks, the
// host-computed tables (source block boundaries, the qualifying columns of each working row, the rotated sampling pattern), the
// stream-ordered scratch, and the launches of kernels_feat.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/vr180_remap.h"
#include "feat_launch.hpp"
#include "host_util.hpp"

using namespace v1c;
using namespace v1c::feat;

#define FEAT_HIP_TRY(expr)                                                                              \
    do {                                                                                                \
        hipError_t _e = (expr);                                                                         \
        if (_e != hipSuccess)                                                                           \
            return set_error(V1C_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));             \
    } while (0)

namespace {

#pragma clang fp contract(off)

// round half away from zero, written out so that the NumPy restatement evaluates the same expression
int round_away(double v)
{
    const double a = std::floor(std::fabs(v) + 0.5);
    return (int)(v < 0 ? -a : a);
}

uint64_t splitmix64(uint64_t& s)
{
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// one coordinate of the base pattern: the Irwin-Hall sum of 12 uniform 16-bit draws (mean 12 * 32767.5, standard deviation ~65536)
// scaled to a standard deviation of 6 pixels and rounded half away from zero -- integer arithmetic only
int gauss_coord(uint64_t& s)
{
    int64_t v = -393210;
    for (int k = 0; k < 12; k++)
        v += (int64_t)(splitmix64(s) >> 48);
    const int64_t n = v * 6;
    return (int)(n >= 0 ? (n + 32768) / 65536 : -((-n + 32768) / 65536));
}

constexpr uint64_t kPatternSeed = 0x5EEDF3A7u;
constexpr int kPatternClip = 13;  // base points within radius 13: every rotated and rounded point stays inside radius 15

// kBins x kPairs x (px, py, qx, qy): the base pattern rotated by the centre angle (2k + 1) * 6 degrees of each sector
void build_pattern(int8_t* out)
{
    int base[kPairs][4];
    uint64_t s = kPatternSeed;
    for (int n = 0; n < kPairs;) {
        int c[4];
        for (int k = 0; k < 4; k++)
            c[k] = gauss_coord(s);
        const bool inside = c[0] * c[0] + c[1] * c[1] <= kPatternClip * kPatternClip && c[2] * c[2] + c[3] * c[3] <= kPatternClip * kPatternClip;
        if (inside && (c[0] != c[2] || c[1] != c[3])) {
            std::memcpy(base[n], c, sizeof(c));
            n++;
        }
    }
    for (int k = 0; k < kBins; k++) {
        const double th = (2 * k + 1) * M_PI / 30;
        const double co = std::cos(th), si = std::sin(th);
        for (int n = 0; n < kPairs; n++)
            for (int e = 0; e < 2; e++) {
                const double x = base[n][2 * e], y = base[n][2 * e + 1];
                out[(k * kPairs + n) * 4 + 2 * e] = (int8_t)round_away(co * x - si * y);
                out[(k * kPairs + n) * 4 + 2 * e + 1] = (int8_t)round_away(si * x + co * y);
            }
    }
}

// b_k = round(2^15 (cos, sin)(12 k degrees))
void build_bin_vectors(int32_t* out)
{
    for (int k = 0; k < kBins; k++) {
        const double th = k * M_PI / 15;
        out[2 * k] = round_away(32768.0 * std::cos(th));
        out[2 * k + 1] = round_away(32768.0 * std::sin(th));
    }
}

constexpr size_t kPatternBytes = (size_t)kBins * kPairs * 4;

// per device: the rotated pattern followed by the boundary vectors, uploaded once
int device_tables(int device, const int8_t** pattern, const int32_t** bv)
{
    static std::mutex mu;
    static std::map<int, void*> tables;
    std::lock_guard<std::mutex> lock(mu);
    void*& d = tables[device];
    if (!d) {
        std::vector<uint8_t> h(kPatternBytes + kBins * 2 * sizeof(int32_t));
        build_pattern((int8_t*)h.data());
        build_bin_vectors((int32_t*)(h.data() + kPatternBytes));
        void* p = nullptr;
        FEAT_HIP_TRY(hipMalloc(&p, h.size()));
        hipError_t e = hipMemcpy(p, h.data(), h.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(p);
            return set_error(V1C_E_HIP, std::string("hipMemcpy (feature pattern): ") + hipGetErrorString(e));
        }
        d = p;
    }
    *pattern = (const int8_t*)d;
    *bv = (const int32_t*)((const uint8_t*)d + kPatternBytes);
    return V1C_OK;
}

}  // namespace

extern "C" int v1c_feat_pattern(int8_t* out)
{
    if (!out)
        return set_error(V1C_E_INVALID, "v1c_feat_pattern: out is NULL");
    build_pattern(out);
    return V1C_OK;
}

extern "C" int v1c_feat_detect(int device, void* stream, const uint8_t* img, int h, int w, int64_t pitch, int cn,
                               const v1c_feat_params* prm, v1c_feat_kp* kp_out, uint8_t* desc_out, int32_t* count_out_dev)
{
    if (!img || !prm || !kp_out || !desc_out || !count_out_dev)
        return set_error(V1C_E_INVALID, "v1c_feat_detect: NULL pointer");
    if (cn != 1 && cn != 3 && cn != 4)
        return set_error(V1C_E_INVALID, "v1c_feat_detect: cn must be 1, 3 or 4");
    if (h <= 0 || w <= 0 || h > 32768 || w > 32768 || pitch < (int64_t)w * cn)
        return set_error(V1C_E_INVALID, "v1c_feat_detect: image size must be 1..32768 with pitch >= w * cn");
    const double s = prm->scale;
    if (!(s > 0.0 && s <= 1.0))
        return set_error(V1C_E_INVALID, "v1c_feat_detect: scale must lie in (0, 1]");
    if (!(prm->radius > 0.0 && prm->radius <= 1e9))
        return set_error(V1C_E_INVALID, "v1c_feat_detect: radius must lie in (0, 1e9]");
    if (prm->fast_threshold < 1 || prm->fast_threshold > 255 || prm->cell < kMinCell || prm->cell > kMaxCell || prm->per_cell < 1 ||
        prm->per_cell > kMaxPerCell || prm->max_keypoints < 1 || prm->max_keypoints > (1 << 20) || prm->margin < 0)
        return set_error(V1C_E_INVALID, "v1c_feat_detect: parameter out of range (fast_threshold 1..255, cell 8..64, per_cell 1..4, "
                                        "max_keypoints 1..2^20, margin >= 0)");
    if (((uintptr_t)desc_out & 7) || ((uintptr_t)kp_out & 3))
        return set_error(V1C_E_INVALID, "v1c_feat_detect: desc_out must be 8-byte and kp_out 4-byte aligned");
    const int ww = (int)(w * s), wh = (int)(h * s);
    if (ww < 2 * kBorder + 1 || wh < 2 * kBorder + 1)
        return set_error(V1C_E_INVALID, "v1c_feat_detect: the working image " + std::to_string(ww) + "x" + std::to_string(wh) +
                                            " is smaller than the pattern needs (33 x 33)");
    // host tables: block boundaries of rows and columns, then the qualifying columns of each working row
    std::vector<int32_t> tab((size_t)(wh + 1) + (ww + 1) + 2 * wh);
    int32_t* rb = tab.data();
    int32_t* cb = rb + wh + 1;
    int32_t* rng = cb + ww + 1;
    for (int i = 0; i <= wh; i++)
        rb[i] = (int32_t)std::min<double>(h, std::floor(i / s));
    for (int i = 0; i <= ww; i++)
        cb[i] = (int32_t)std::min<double>(w, std::floor(i / s));
    for (int i = 0; i < wh; i++)
        if (rb[i + 1] <= rb[i])
            return set_error(V1C_E_INVALID, "v1c_feat_detect: empty source row block");
    for (int i = 0; i < ww; i++)
        if (cb[i + 1] <= cb[i])
            return set_error(V1C_E_INVALID, "v1c_feat_detect: empty source column block");
    const double cx = (double)(w / 2) * s, cy = (double)(h / 2) * s;
    const double R = prm->radius * s - prm->margin;
    bool any = false;
    for (int y = 0; y < wh; y++) {
        // rows and columns within kBorder of the image edge never qualify: FAST reads 3 pixels around a candidate, NMS 1, the
        // orientation disc and the pattern 15 -- whatever the radius (a landscape frame, a clipped circle) and the margin
        int lo = 1, hi = 0;
        const double dy = y - cy;
        const double t = R * R - dy * dy;
        if (y >= kBorder && y <= wh - 1 - kBorder && R >= 0 && t >= 0) {
            const double half = std::sqrt(t);
            const double l = std::max<double>(std::ceil(cx - half), kBorder);
            const double u = std::min<double>(std::floor(cx + half), ww - 1 - kBorder);
            if (l <= u) {
                lo = (int)l;
                hi = (int)u;
                any = true;
            }
        }
        rng[2 * y] = lo;
        rng[2 * y + 1] = hi;
    }
    if (!any)
        return set_error(V1C_E_INVALID, "v1c_feat_detect: empty circle (no working pixel lies within radius * scale - margin of the "
                                        "centre and off the border)");

    DeviceGuard dg(device);
    if (!dg.ok)
        return set_error(V1C_E_NODEVICE, "hipSetDevice failed");
    DetectArgs a{};
    int rc = device_tables(device, &a.pattern, &a.bv);
    if (rc)
        return rc;
    hipStream_t st = (hipStream_t)stream;
    const int ncx = (ww + prm->cell - 1) / prm->cell, ncy = (wh + prm->cell - 1) / prm->cell;
    const size_t px = (size_t)ww * wh, nslots = (size_t)ncx * ncy * prm->per_cell;
    const size_t o_sm = align256(px), o_score = o_sm + align256(px), o_tab = o_score + align256(px);
    const size_t o_cand = o_tab + align256(tab.size() * sizeof(int32_t)), o_hist = o_cand + align256(nslots * 4);
    const size_t bytes = o_hist + 256 * 4;
    uint8_t* ws = nullptr;
    FEAT_HIP_TRY(hipMallocAsync((void**)&ws, bytes, st));
    a.src = img;
    a.pitch = pitch;
    a.cn = cn;
    a.h = h;
    a.w = w;
    a.wh = wh;
    a.ww = ww;
    a.rb = (const int32_t*)(ws + o_tab);
    a.cb = a.rb + wh + 1;
    a.rng = a.cb + ww + 1;
    a.threshold = prm->fast_threshold;
    a.cell = prm->cell;
    a.per_cell = prm->per_cell;
    a.max_kp = prm->max_keypoints;
    a.y = ws;
    a.sm = ws + o_sm;
    a.score = ws + o_score;
    a.cand = (uint32_t*)(ws + o_cand);
    a.hist = (uint32_t*)(ws + o_hist);
    a.kp = (Kp*)kp_out;
    a.desc = desc_out;
    a.count = count_out_dev;
    hipError_t e = hipMemcpyAsync(ws + o_tab, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = hipMemsetAsync(a.hist, 0, 256 * 4, st);
    if (e == hipSuccess)
        e = launch_detect(a, st);
    const hipError_t ef = hipFreeAsync(ws, st);
    if (e != hipSuccess)
        return set_error(V1C_E_HIP, std::string("v1c_feat_detect: ") + hipGetErrorString(e));
    FEAT_HIP_TRY(ef);
    return V1C_OK;
}

extern "C" int v1c_feat_match(int device, void* stream, const uint8_t* desc_a, int n_a, const uint8_t* desc_b, int n_b,
                              const v1c_feat_params* prm, int32_t* pairs_out, int32_t* dist_out, int32_t* count_out_dev)
{
    if (!prm || !pairs_out || !dist_out || !count_out_dev || (n_a > 0 && !desc_a) || (n_b > 0 && !desc_b))
        return set_error(V1C_E_INVALID, "v1c_feat_match: NULL pointer");
    if (n_a < 0 || n_b < 0 || n_a > (1 << 24) || n_b > (1 << 24))
        return set_error(V1C_E_INVALID, "v1c_feat_match: descriptor counts must be 0..2^24");
    if (((uintptr_t)desc_a & 15) || ((uintptr_t)desc_b & 15))
        return set_error(V1C_E_INVALID, "v1c_feat_match: descriptor arrays must be 16-byte aligned");
    if (prm->max_distance < 0 || prm->max_distance > 256 || prm->ratio_num < 0 || prm->ratio_num > 1024 || prm->ratio_den < 1 ||
        prm->ratio_den > 1024)
        return set_error(V1C_E_INVALID, "v1c_feat_match: max_distance must be 0..256, ratio_num 0..1024, ratio_den 1..1024");
    DeviceGuard dg(device);
    if (!dg.ok)
        return set_error(V1C_E_NODEVICE, "hipSetDevice failed");
    hipStream_t st = (hipStream_t)stream;
    if (n_a == 0 || n_b == 0) {
        FEAT_HIP_TRY(hipMemsetAsync(count_out_dev, 0, sizeof(int32_t), st));
        return V1C_OK;
    }
    void* ws = nullptr;
    FEAT_HIP_TRY(hipMallocAsync(&ws, match_scratch_bytes(n_a, n_b), st));
    const hipError_t e = launch_match(desc_a, n_a, desc_b, n_b, prm->max_distance, prm->ratio_num, prm->ratio_den, ws, pairs_out,
                                      dist_out, count_out_dev, st);
    const hipError_t ef = hipFreeAsync(ws, st);
    if (e != hipSuccess)
        return set_error(V1C_E_HIP, std::string("v1c_feat_match: ") + hipGetErrorString(e));
    FEAT_HIP_TRY(ef);
    return V1C_OK;
}
