// jpeg_launch.hpp -- the buffer set of the JPEG encoder's kernels and the launcher of the single call's (kernels_jpeg.hip), called by
// the C ABI in jpeg.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jpeg_core.hpp"

namespace v1c {
namespace jpeg {

constexpr uint32_t kScanChunk = 2048;  // entries one workgroup of the scans takes

// The buffers the stages hand on to each other, for one image (Args) or for the images of a chunk, every image's region back to back
// (Batch, jpeg_batch.hpp).  The stages' bodies (jpeg_kernels.hpp) know no more of their caller than this.
struct Buffers {
    int16_t* coef;       // nblocks x 64 quantised coefficients in zigzag order, MCU-major
    uint32_t* bits;      // coded bits of every block
    uint64_t* bitoff;    // nblocks + 1: their exclusive scan
    uint32_t* ibytes;    // bytes of every interval with its pad, before stuffing
    uint64_t* ioff;      // nint + 1: their exclusive scan
    uint32_t* raw;       // the intervals back to back before stuffing, zeroed; whole pieces, an image's region starts on one
    uint32_t* ffcnt;     // 0xFF bytes of every kPiece bytes of raw
    uint64_t* ffoff;     // pieces + 1: their exclusive scan
    uint64_t* sums;      // the scans' per-chunk sums
    uint8_t* out;        // the scans: stuffed intervals and RSTm markers
};

struct Args {
    const uint8_t* img;
    int64_t pitch;
    Geom g;
    const Tables* tab;
    Buffers buf;
    uint64_t* total;     // the scan's size
};

// every kernel of one image, in order, on `st`; nothing synchronises
hipError_t launch_encode(const Args& a, hipStream_t st);

// the exclusive scan the encoder's passes are joined by, for the decoder too (kernels_jpegdec.hip): out[i] = the sum of in[0 .. i),
// out[n] = the total; sums: one word per kScanChunk entries
hipError_t launch_scan(const uint32_t* in, uint64_t n, uint64_t* sums, uint64_t* out, hipStream_t st);

}  // namespace jpeg
}  // namespace v1c
