// feat_launch.hpp -- launchers of the feature kernels (kernels_feat.hip), called by the C ABI in feat.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "feat_core.hpp"

namespace v1c {
namespace feat {

// one keypoint record as v1c_feat_kp lays it out (include/vr180_remap.h)
struct Kp {
    int32_t x, y, score, bin, src_x2, src_y2;
};

struct DetectArgs {
    const uint8_t* src;
    int64_t pitch;
    int cn, h, w;           // source image
    int wh, ww;             // working image
    const int32_t* rb;      // wh + 1 source row boundaries of the working rows
    const int32_t* cb;      // ww + 1 source column boundaries
    const int32_t* rng;     // wh (lo, hi) pairs: the qualifying columns of each working row
    const int8_t* pattern;  // kBins x kPairs x (px, py, qx, qy)
    const int32_t* bv;      // kBins (x, y) orientation boundary vectors
    int threshold, cell, per_cell, max_kp;
    uint8_t* y;             // working images: luma, smoothed, candidate scores (wh x ww each)
    uint8_t* sm;
    uint8_t* score;
    uint32_t* cand;         // ncell * per_cell ranking keys
    uint32_t* hist;         // 256 score counts
    Kp* kp;
    uint8_t* desc;
    int32_t* count;
};

hipError_t launch_detect(const DetectArgs& a, hipStream_t st);

// brute-force match of n_a against n_b descriptors, both directions; `part` / `best` scratch sized by match_scratch_bytes
size_t match_scratch_bytes(int n_a, int n_b);
hipError_t launch_match(const uint8_t* da, int n_a, const uint8_t* db, int n_b, int d_max, int num, int den, void* scratch,
                        int32_t* pairs, int32_t* dist, int32_t* count, hipStream_t st);

}  // namespace feat
}  // namespace v1c
