// jpegprog_launch.hpp -- launchers of the progressive JPEG decoder's kernels (kernels_jpegprog.hip), called by the C ABI in jpegdec.hip
// once per scan of the file.  Unstuffing in front of them and the pixel stage behind the last scan are the sequential decoder's
// (jpegdec_launch.hpp: launch_unstuff, launch_pixels).
#pragma once

#include <hip/hip_runtime.h>

#include "jpegprog_core.hpp"

namespace v1c {
namespace jpegprog {

// exit[0] = the grid states, last = none
hipError_t launch_init(const ScanArgs& a, hipStream_t st);
// round r = 1, 2, ...: exit[r & 1] = F(entry by exit[(r - 1) & 1]); flags[r & 1] is raised where an entry state changed, flags[(r + 1) & 1] cleared
hipError_t launch_round(const ScanArgs& a, uint32_t r, hipStream_t st);
// after the last round r: the block-count scan and the last pass into the store, flags[2] gets the first error bit; behind a DC first
// scan the scan of the differences and the values' way into the store
hipError_t launch_write(const ScanArgs& a, uint32_t r, hipStream_t st);
// behind the last scan: the store's DC values to the differences the sequential pixel stage takes
hipError_t launch_dcdiff(const ScanArgs& a, hipStream_t st);

}  // namespace jpegprog
}  // namespace v1c
