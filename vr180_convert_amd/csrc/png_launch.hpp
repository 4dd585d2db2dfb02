// png_launch.hpp -- launchers of the PNG encoder's kernels (kernels_png.hip), called by the C ABI in png.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "png_core.hpp"

namespace v1c {
namespace png {

struct Args {
    const uint8_t* img;
    int64_t pitch;
    uint32_t h, stride;         // rows; bytes of a scanline with its filter byte
    int filter;
    uint32_t band_rows, n_bands;
    uint32_t segs_per_band;     // of a full band: segment k of band b has the global index b * segs_per_band + k
    uint32_t groups;            // workgroups per band
    uint32_t* hist;             // n_bands x kHistStride symbol counts
    unsigned long long* adler;  // n_bands x (sum of bytes, sum of (n - i) * byte[i] reduced modulo 65521 per wave)
    const BandDev* bands;
    const uint32_t* tables;     // n_bands x kSymbols code table entries
    uint32_t* segbits;          // bits of every segment's tokens
    uint64_t* segoff;           // bit of the stream at which every segment starts
    uint32_t* out;              // the stream, zeroed
};

hipError_t launch_pass1(const Args& a, int bpp, hipStream_t st);
hipError_t launch_pass2(const Args& a, int bpp, bool any_coded, bool any_stored, const OrWord* list, uint32_t n_or, hipStream_t st);

}  // namespace png
}  // namespace v1c
