// jpegxc_launch.hpp -- launchers of the lossless JPEG transcoder (kernels_jpegxc.hip), called by the C ABI in jpegxc.hip and by the
// lossless entries' chain (jpegx_chain.hpp): the DC scan
// of a decoded file without its pixel stage, the gather of an output's blocks from the decoder's coefficient store into the encoder's,
// and the encoder's chain from a filled coefficient store on.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jpeg_batch.hpp"
#include "jpeg_opt_kernels.hpp"
#include "jpegdec_launch.hpp"
#include "jpegxc_core.hpp"

namespace v1c {
namespace jpegxc {

struct GatherArgs {
    const int16_t* src;      // the decoder's store: the source's nblocks x 64, zigzag order, MCU-major, the DC a difference
    const uint64_t* dcoff;   // the decoder's DC scan (launch_dc)
    jpegdec::Geom sg;        // the source's geometry
    int16_t* dst;            // the output's blocks in the encoder's store: the same layout, the DC a value
    uint32_t dst_mcux;       // MCUs of a row of the output
    uint32_t dst_nblocks;
    uint32_t* flag;          // raised where a coefficient is none the encoder's tables code (jpegxc_core.hpp: codable)
    RegionList regions;
};

// the decoder's DC differences by component and their scan into a.dcoff: the first two steps of its pixel stage, and no more
hipError_t launch_dc(const jpegdec::Args& a, hipStream_t st);

// one output's blocks; nothing synchronises
hipError_t launch_gather(const GatherArgs& a, hipStream_t st);

// The encoder's chain of a chunk whose coefficient store is filled, from `size` on, with the histograms and the table builder in front
// where o is not NULL.  The size, pack and histogram stages are this code object's (any number of luma blocks per MCU); the interval,
// count and place stages, the scans and the builder are the encoder's own kernels, launched as they are.  first_host: the host's copy of the work lists
hipError_t launch_encode_coef(const jpeg::Batch& b, const jpeg::OptBatch* o, const uint32_t* first_host, hipStream_t st);

}  // namespace jpegxc
}  // namespace v1c
