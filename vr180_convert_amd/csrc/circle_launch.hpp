// circle_launch.hpp -- launcher of the image-circle kernels (kernels_circle.hip), called by the C ABI in circle.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "circle_core.hpp"

namespace v1c {
namespace circle {

// the caller's workspace: 2 (h + w) point slots (uint32: rows' left / right ends, then columns' top / bottom ends) and, 256-byte
// aligned behind them, one selection flag (uint8) per slot, then 256 bytes where the synchronous entry keeps its eight doubles, then
// the columns' band records
inline size_t slots(int h, int w) { return 2 * ((size_t)h + (size_t)w); }
inline size_t flags_offset(int h, int w) { return (slots(h, w) * 4 + 255) & ~(size_t)255; }
inline size_t result_offset(int h, int w) { return flags_offset(h, w) + ((slots(h, w) + 255) & ~(size_t)255); }
inline int bands(int h) { return (h + kBandRows - 1) / kBandRows; }
inline size_t bands_offset(int h, int w) { return result_offset(h, w) + 256; }  // the columns' band records: bands(h) x w uint32
inline size_t workspace_bytes(int h, int w) { return bands_offset(h, w) + (((size_t)bands(h) * w * 4 + 255) & ~(size_t)255); }

// rows, column bands, column join, fit: four launches on `st`, nothing else.  depth16: uint16 pixels (pitch stays in BYTES).
hipError_t launch_fit(const uint8_t* img, int h, int w, int64_t pitch, int cn, bool depth16, const Params& prm, uint8_t* workspace,
                      double* out8, hipStream_t st);

}  // namespace circle
}  // namespace v1c
