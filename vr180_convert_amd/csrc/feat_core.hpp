// feat_core.hpp -- per-pixel and per-keypoint arithmetic of the feature pipeline (kernels_feat.hip, feat.hip).
//
// __host__ __device__ so that tests/host_feat/feat_emul.hip runs exactly this code on the host against the NumPy restatement
// (tests/feat_ref.py).  Integer arithmetic throughout: the contract is bit-exactness from input bytes to match list
// ("Feature matching").
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace v1c {
namespace feat {

constexpr int kPatchRadius = 15;           // orientation disc; the sampling pattern stays inside it
constexpr int kBorder = kPatchRadius + 1;  // keypoints keep this far from the working image's edges (disc + the NMS neighbours)
constexpr int kPairs = 256;                // descriptor bits
constexpr int kBins = 30;                  // orientation sectors of 12 degrees
constexpr int kDescBytes = kPairs / 8;
constexpr int kMaxPerCell = 4;
constexpr int kMinCell = 8, kMaxCell = 64;
constexpr int kNoSecond = 0x7fff;          // second-best distance of a query with a single candidate

// BT.601 luma in Q14 of one B,G,R(,A) / grey pixel
__host__ __device__ inline int luma(const uint8_t* px, int cn)
{
    if (cn == 1)
        return px[0];
    return (1868 * px[0] + 9617 * px[1] + 4899 * px[2] + 8192) >> 14;
}

// round-half-up integer mean of `cnt` values summing to `sum`
__host__ __device__ inline int block_mean(int sum, int cnt)
{
    return (2 * sum + cnt) / (2 * cnt);
}

// one pass of the [1 4 6 4 1] / 16 binomial
__host__ __device__ inline int smooth5(int a, int b, int c, int d, int e)
{
    return (a + 4 * b + 6 * c + 4 * d + e + 8) >> 4;
}

// the 16-pixel Bresenham circle of radius 3, clockwise from the top
__host__ __device__ inline int circle_dx(int k)
{
    constexpr int dx[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
    return dx[k];
}
__host__ __device__ inline int circle_dy(int k)
{
    constexpr int dy[16] = {-3, -3, -2, -1, 0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3};
    return dy[k];
}

// FAST-9 score at (x, y) of an 8-bit image: the maximum, over the 32 (start, sign) arcs of 9 contiguous circle pixels, of the minimum
// signed difference along the arc.  The caller keeps (x, y) at least 3 pixels inside the image.
__host__ __device__ inline int fast_score(const uint8_t* img, int64_t pitch, int x, int y)
{
    const int c = img[(int64_t)y * pitch + x];
    int d[16];
#pragma unroll
    for (int k = 0; k < 16; k++)
        d[k] = img[(int64_t)(y + circle_dy(k)) * pitch + x + circle_dx(k)] - c;
    int best = -256;
#pragma unroll
    for (int s = 0; s < 16; s++) {
        int lo = 256, hi = -256;  // min and max of d along the arc: the brighter arc scores lo, the darker one -hi
#pragma unroll
        for (int k = 0; k < 9; k++) {
            const int v = d[(s + k) & 15];
            lo = lo < v ? lo : v;
            hi = hi > v ? hi : v;
        }
        best = best > lo ? best : lo;
        best = best > -hi ? best : -hi;
    }
    return best;
}

// 3 x 3 non-maximum suppression on (score, -y, -x): `s` is the candidate score map (0 = no candidate), (x, y) a candidate at least one
// pixel inside it.  Kept iff it beats every candidate neighbour lexicographically.
__host__ __device__ inline bool nms_keep(const uint8_t* s, int64_t pitch, int x, int y)
{
    const int c = s[(int64_t)y * pitch + x];
    bool keep = true;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++)
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            if (dx == 0 && dy == 0)
                continue;
            const int v = s[(int64_t)(y + dy) * pitch + x + dx];
            // the neighbour wins on a higher score, or on an equal one when it comes first in (y, x) order
            const bool before = dy < 0 || (dy == 0 && dx < 0);
            keep &= !(v > c || (v == c && before));
        }
    return keep;
}

// cell-local ranking key: larger = earlier in (score desc, y, x); p = the pixel's row-major index inside its cell (< 65536); 0 = none
__host__ __device__ inline uint32_t cell_key(int score, int p)
{
    return ((uint32_t)score << 16) | (uint32_t)(0xffff - p);
}
__host__ __device__ inline int key_score(uint32_t key) { return (int)(key >> 16); }
__host__ __device__ inline int key_pixel(uint32_t key) { return 0xffff - (int)(key & 0xffff); }

// offset i in [0, 31 * 31) of the square around a keypoint; true iff it lies on the radius-15 disc
__host__ __device__ inline bool disc_offset(int i, int* dx, int* dy)
{
    *dx = i % (2 * kPatchRadius + 1) - kPatchRadius;
    *dy = i / (2 * kPatchRadius + 1) - kPatchRadius;
    return *dx * *dx + *dy * *dy <= kPatchRadius * kPatchRadius;
}

// orientation sector of the moment vector (m10, m01): the k with cross(b_k, m) >= 0 > cross(b_{k+1}, m), b_k = round(2^15 (cos, sin)
// of 12 k degrees) -- `bv`: kBins (x, y) pairs; (0, 0) gives 0
__host__ __device__ inline int orient_bin(int m10, int m01, const int32_t* bv)
{
    int bin = 0;
    for (int k = kBins - 1; k >= 0; k--) {
        const int k1 = k + 1 == kBins ? 0 : k + 1;
        const int64_t c0 = (int64_t)bv[2 * k] * m01 - (int64_t)bv[2 * k + 1] * m10;
        const int64_t c1 = (int64_t)bv[2 * k1] * m01 - (int64_t)bv[2 * k1 + 1] * m10;
        if (c0 >= 0 && c1 < 0)
            bin = k;
    }
    return bin;
}

// Hamming distance of two 32-byte descriptors held as 8 dwords
__host__ __device__ inline int hamming256(const uint32_t* a, const uint32_t* b)
{
    int d = 0;
#pragma unroll
    for (int k = 0; k < 8; k++)
        d += __builtin_popcount(a[k] ^ b[k]);
    return d;
}

// running (best distance, its index, second-best distance) of one query: candidates in ascending index order, ties keep the lower
// index (and make d2 == d1)
struct Best {
    int d1, idx, d2, pad;
};
__host__ __device__ inline Best best_init()
{
    return Best{kNoSecond, -1, kNoSecond, 0};
}
__host__ __device__ inline void best_push(Best& b, int d, int j)
{
    if (d < b.d1) {
        b.d2 = b.d1;
        b.d1 = d;
        b.idx = j;
    } else if (d < b.d2) {
        b.d2 = d;
    }
}
// merge of two partial results, `lo` over lower candidate indices than `hi`
__host__ __device__ inline Best best_merge(Best lo, Best hi)
{
    Best r;
    if (hi.d1 < lo.d1) {
        r.d1 = hi.d1;
        r.idx = hi.idx;
        r.d2 = lo.d1 < hi.d2 ? lo.d1 : hi.d2;
    } else {
        r.d1 = lo.d1;
        r.idx = lo.idx;
        r.d2 = hi.d1 < lo.d2 ? hi.d1 : lo.d2;
    }
    r.pad = 0;
    return r;
}

// the match rule for query i whose best candidate has result `bj`: mutual best, d1 <= d_max, den * d1 <= num * d2
__host__ __device__ inline bool match_keep(const Best& bi, const Best& bj, int i, int d_max, int num, int den)
{
    return bj.idx == i && bi.d1 <= d_max && den * bi.d1 <= num * bi.d2;
}

}  // namespace feat
}  // namespace v1c
