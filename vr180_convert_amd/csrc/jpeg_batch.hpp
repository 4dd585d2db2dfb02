// jpeg_batch.hpp -- what the batched JPEG encoder (v1c_jpeg_encode_batch: jpeg.hip, kernels_jpeg_batch.hip) adds to the single call,
// and nothing of the arithmetic: every image's regions in the concatenated buffers, the work lists that map a workgroup to its
// image, the values that turn a scan over the concatenation into the single call's, and the cut of a list into chunks under a
// workspace budget.  DESIGN.md section 16.
//
// The values relative to an image are what the stages' bodies (jpeg_kernels.hpp) compute with for the single call too, whose image has
// its regions at zero.  __host__ __device__ / plain C++ so that tests/host_jpeg_batch/ runs exactly this code in its sequential copy of
// the kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "jpeg_core.hpp"
#include "jpeg_launch.hpp"
#include "jpegdec_batch.hpp"

namespace v1c {
namespace jpeg {

using jpegdec::chunk_ends;  // images in order under a budget of bytes and of 2^31 - 1 workgroups; a larger image is a chunk of its own
using jpegdec::file_of;     // the image of a workgroup: the last f with first[f] <= wg, in 32 halvings at the most

// The work lists of a chunk of n images, one per grid shape: first[list * (n + 1) + f] is the first workgroup of image f in that list's
// kernels, [.. + n] their number.  No workgroup spans two images.
enum WorkList { kByTile = 0, kByBlock = 1, kByPiece = 2, kWorkLists = 3 };  // 32 blocks; 256 blocks or intervals; 256 pieces of raw

// the decoder's default (jpegdec::kDefaultBatchWorkspace): the encoder's workspace is of the same order per pixel
constexpr uint64_t kDefaultBatchWorkspace = (uint64_t)1 << 30;

// One image of a chunk.  Its regions keep the single call's layout at the single call's worst-case sizes and lie back to back with
// the other images': g.nblocks entries of coef / bits from blk0, g.nint of ibytes from int0, pieces_of(g) pieces of raw (and entries
// of ffcnt) from piece0, scan_bound(g) bytes of out from out0.
struct Image {
    const uint8_t* img;
    int64_t pitch;
    Geom g;
    uint32_t tab;  // its quality's entry of the chunk's Tables
    uint64_t blk0, int0, piece0, out0;
};

__host__ __device__ inline uint64_t pieces_of(const Geom& g)
{
    return raw_bound(g) / kPiece;
}

__host__ __device__ inline uint64_t groups_of(const Geom& g, int list)
{
    const uint64_t n = list == kByPiece ? pieces_of(g) : g.nblocks, per = list == kByTile ? 32 : 256;
    return (n + per - 1) / per;
}

// the concatenated buffers' entries
struct Totals {
    uint64_t nblocks = 0, nint = 0, pieces = 0, out_bytes = 0;
};

// the regions of images whose geometry is set, in order, and the work lists (kWorkLists * (n + 1) words)
inline Totals place_regions(Image* im, uint32_t n, uint32_t* first)
{
    Totals t;
    for (int l = 0; l < kWorkLists; l++)
        first[(size_t)l * (n + 1)] = 0;
    for (uint32_t f = 0; f < n; f++) {
        const Geom& g = im[f].g;
        im[f].blk0 = t.nblocks, im[f].int0 = t.nint, im[f].piece0 = t.pieces, im[f].out0 = t.out_bytes;
        t.nblocks += g.nblocks, t.nint += g.nint, t.pieces += pieces_of(g), t.out_bytes += scan_bound(g);
        for (int l = 0; l < kWorkLists; l++)
            first[(size_t)l * (n + 1) + f + 1] = first[(size_t)l * (n + 1) + f] + (uint32_t)groups_of(g, l);
    }
    return t;
}

// entries of the scans' per-chunk sums that a chunk needs (scan_chunk: kScanChunk of jpeg_launch.hpp)
inline uint64_t sums_of(const Totals& t, uint32_t scan_chunk)
{
    uint64_t m = t.nblocks > t.pieces ? t.nblocks : t.pieces;
    m = m > t.nint ? m : t.nint;
    return (m + scan_chunk - 1) / scan_chunk + 1;
}

// Bytes of device workspace an image adds to its chunk, for the cut into chunks: its regions, its share of the scans' sums and of the
// chunk's head (descriptor, work lists, tables, size), and what the alignment of the buffers can add.
inline uint64_t workspace_of(const Geom& g)
{
    const uint64_t p = pieces_of(g);
    return (uint64_t)g.nblocks * (128 + 4 + 8) + (uint64_t)g.nint * (4 + 8) + p * (kPiece + 4 + 8) + scan_bound(g) +
           ((p > g.nblocks ? p : g.nblocks) / 2048 + 2) * 8 + sizeof(Image) + sizeof(Tables) + kWorkLists * 4 + 8 + 4096;
}

// the largest number of workgroups the image has in any list
inline uint64_t most_groups(const Geom& g)
{
    uint64_t m = 0;
    for (int l = 0; l < kWorkLists; l++)
        m = groups_of(g, l) > m ? groups_of(g, l) : m;
    return m;
}

// ---- what turns a scanned value of the concatenation into the single call's ------------------------------------------------------------

// the DC that block b of the image is predicted from: 0 for the first block of each component of an interval, so of the image too,
// whatever lies in front of it in the concatenated coef
__host__ __device__ inline int dc_prediction(const Image& im, const int16_t* coef, uint32_t b)
{
    const uint32_t p = dc_predecessor(im.g, b);
    return p == b ? 0 : coef[(size_t)(im.blk0 + p) * 64];
}

// bytes of interval i of the image before stuffing, with its pad
__host__ __device__ inline uint32_t interval_bytes(const Image& im, const uint64_t* bitoff, uint32_t i)
{
    const uint64_t f = (uint64_t)i * im.g.ibl, e = f + im.g.ibl < im.g.nblocks ? f + im.g.ibl : im.g.nblocks;
    return (uint32_t)((bitoff[im.blk0 + e] - bitoff[im.blk0 + f] + 7) >> 3);
}

// the byte of the image's unstuffed stream at which interval i <= g.nint starts (g.nint: the stream's length)
__host__ __device__ inline uint64_t interval_start(const Image& im, const uint64_t* ioff, uint32_t i)
{
    return ioff[im.int0 + i] - ioff[im.int0];
}

// the bit of the image's unstuffed stream at which block b starts
__host__ __device__ inline uint64_t block_bit(const Image& im, const uint64_t* bitoff, const uint64_t* ioff, uint32_t b)
{
    const uint32_t iv = b / im.g.ibl;
    return 8 * interval_start(im, ioff, iv) + (bitoff[im.blk0 + b] - bitoff[im.blk0 + (uint64_t)iv * im.g.ibl]);
}

// the 0xFF bytes of the image in front of its piece p
__host__ __device__ inline uint64_t ff_before(const Image& im, const uint64_t* ffoff, uint64_t p)
{
    return ffoff[im.piece0 + p] - ffoff[im.piece0];
}

// the second byte of the marker behind interval iv of an image: RSTm counts from the image's own first interval
__host__ __device__ inline uint8_t rst_marker(uint32_t iv)
{
    return (uint8_t)(0xd0 + (iv & 7u));
}

// ---- the kernels' arguments ------------------------------------------------------------------------------------------------------------
struct Batch {
    const Image* im;
    const uint32_t* first;  // the work lists
    const Tables* tabs;     // one per distinct quality of the chunk
    uint32_t n;
    Totals t;
    Buffers buf;            // every image's region back to back; bitoff, ioff and ffoff are the scans over all images' entries
    uint64_t* sizes;        // n: every image's scan size, zeroed
};

// every kernel of a chunk, in order, on `st`; nothing synchronises.  first_host: the host's copy of the work lists
hipError_t launch_encode_batch(const Batch& b, const uint32_t* first_host, hipStream_t st);

}  // namespace jpeg
}  // namespace v1c
