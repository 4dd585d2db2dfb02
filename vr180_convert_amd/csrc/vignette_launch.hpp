// vignette_launch.hpp -- launchers of the vignetting kernels (kernels_vignette.hip), called by the C ABI in vignette.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vignette_core.hpp"

namespace v1c {
namespace vignette {

// one launch on `st`; dst may be src.  es: bytes of an element (1, 2)
hipError_t launch_apply(const uint8_t* src, int64_t pitch_s, uint8_t* dst, int64_t pitch_d, int h, int w, int cn, int es, const Geom& geom,
                        const uint16_t* tables, hipStream_t st);

// the record zeroed and the statistics: two launches on `st`, nothing else.  rings: prm.rings x 4 int64
hipError_t launch_rings(const uint8_t* src, int64_t pitch, int h, int w, int cn, int es, const RingParams& prm, int64_t* rings, hipStream_t st);

}  // namespace vignette
}  // namespace v1c
