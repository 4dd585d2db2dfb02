// colormatch_launch.hpp -- launchers of the colour-match kernels (kernels_colormatch.hip), called by the C ABI in colormatch.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "colormatch_core.hpp"

namespace v1c {
namespace colormatch {

// the caller's workspace: the histograms h[eye][channel][bin], uint32
inline size_t workspace_bytes() { return kHistWords * sizeof(uint32_t); }

// the workspace zeroed, the histograms, the tables and the report: three launches on `st`, nothing else
hipError_t launch_luts(const uint8_t* left, int64_t pitch_l, const uint8_t* right, int64_t pitch_r, int h, int w, int cn, const Params& prm,
                       uint32_t* workspace, uint8_t* luts, int32_t* report, hipStream_t st);

// one launch on `st`; dst may be src
hipError_t launch_apply(const uint8_t* src, int64_t pitch_s, uint8_t* dst, int64_t pitch_d, int h, int w, int cn, const uint8_t* luts,
                        hipStream_t st);

}  // namespace colormatch
}  // namespace v1c
