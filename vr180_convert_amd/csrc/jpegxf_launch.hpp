// jpegxf_launch.hpp -- launcher of the lossless JPEG composer's gather (kernels_jpegxf.hip), called by the C ABI in jpegxf.hip: the
// blocks of one output from the coefficient stores of up to four decoded files, rotated, flipped or transposed on the way.  The decode
// in front of it and the encoder's chain behind it are the transcoder's launchers (jpegxc_launch.hpp), as they are.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jpegdec_core.hpp"
#include "jpegxf_core.hpp"

namespace v1c {
namespace jpegxf {

struct GatherSource {
    const int16_t* coef;     // the decoder's store of the file: nblocks x 64, zigzag order, MCU-major, the DC a difference
    const uint64_t* dcoff;   // its DC scan (jpegxc::launch_dc)
    jpegdec::Geom g;
};

struct GatherArgs {
    GatherSource src[kMaxSources];
    int16_t* dst;            // the output's blocks in the encoder's store: the same layout, the DC a value
    uint32_t dst_mcux;       // MCUs of a row of the output
    uint32_t dst_nblocks;
    uint32_t* flag;          // raised where a coefficient is none the encoder's tables code (jpegxc_core.hpp: codable)
    RegionList regions;
};

// one output's blocks; nothing synchronises
hipError_t launch_gather(const GatherArgs& a, hipStream_t st);

}  // namespace jpegxf
}  // namespace v1c
