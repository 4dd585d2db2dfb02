// jpeg_launch.hpp -- launcher of the JPEG encoder's kernels (kernels_jpeg.hip), called by the C ABI in jpeg.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jpeg_core.hpp"

namespace v1c {
namespace jpeg {

constexpr uint32_t kScanChunk = 2048;  // entries one workgroup of the scans takes

struct Args {
    const uint8_t* img;
    int64_t pitch;
    Geom g;
    const Tables* tab;
    int16_t* coef;       // nblocks x 64 quantised coefficients in zigzag order, MCU-major
    uint32_t* bits;      // coded bits of every block
    uint64_t* bitoff;    // nblocks + 1: their exclusive scan
    uint32_t* ibytes;    // bytes of every interval with its pad, before stuffing
    uint64_t* ioff;      // nint + 1: their exclusive scan
    uint32_t* raw;       // the intervals back to back before stuffing, zeroed; raw_bound bytes
    uint32_t* ffcnt;     // 0xFF bytes of every kPiece bytes of raw
    uint64_t* ffoff;     // pieces + 1: their exclusive scan
    uint64_t* sums;      // the scans' per-chunk sums
    uint8_t* out;        // the scan: stuffed intervals and RSTm markers
    uint64_t* total;     // its size
};

// every kernel of one image, in order, on `st`; nothing synchronises
hipError_t launch_encode(const Args& a, hipStream_t st);

// the exclusive scan the encoder's passes are joined by, for the decoder too (kernels_jpegdec.hip): out[i] = the sum of in[0 .. i),
// out[n] = the total; sums: one word per kScanChunk entries
hipError_t launch_scan(const uint32_t* in, uint64_t n, uint64_t* sums, uint64_t* out, hipStream_t st);

}  // namespace jpeg
}  // namespace v1c
