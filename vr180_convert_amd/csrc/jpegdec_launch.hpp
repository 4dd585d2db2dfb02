// jpegdec_launch.hpp -- launchers of the JPEG decoder's kernels (kernels_jpegdec.hip), called by the C ABI in jpegdec.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jpeg_launch.hpp"
#include "jpegdec_core.hpp"

namespace v1c {
namespace jpegdec {

constexpr uint32_t kNoError = 0xffffffffu;

struct Args {
    Geom g;
    const Tables* tab;
    const uint8_t* scan;     // the stuffed scan and the two bytes of the marker behind it, then zeros up to a whole piece and one more
    uint32_t scan_len;
    uint32_t pieces;         // of kPiece bytes
    uint32_t* drop;          // bytes every piece drops
    uint64_t* dropoff;       // pieces + 1: their exclusive scan
    uint32_t* u;             // the unstuffed stream in whole words, zeroed, two words behind its last byte
    const uint32_t* segoff;  // nseg + 1: its bytes where every segment begins
    const uint32_t* subfirst;  // nseg + 1: the first subsequence of every segment
    uint32_t nsub, S;
    State* exit[2];          // nsub each: what F_i gave in the last round and in the one before
    State* last;             // the entry state F_i was last computed for
    uint32_t* count;         // the blocks it completed
    uint64_t* first;         // nsub + 1: their exclusive scan
    uint32_t* flags;         // [0], [1]: whether a round changed an entry state, by the round's parity; [2]: the last pass's first error bit
    int16_t* coef;           // nblocks x 64, zigzag order, MCU-major, zeroed
    uint32_t* dcd;           // the DC differences ordered by component
    uint64_t* dcoff;         // nblocks + 1: their exclusive scan (modulo 2^32 is what counts)
    uint64_t* sums;          // the scans' per-chunk sums
    uint8_t* plane[3];       // the component planes, padded to whole MCUs
    uint8_t* out;
    int64_t pitch;
    uint32_t out_cn;         // 1 or 3
};

// unstuffing: drop counts, their scan, and the compaction to a.u.  Nothing synchronises.
hipError_t launch_unstuff(const Args& a, hipStream_t st);
// exit[0] = the grid states, last = none
hipError_t launch_sync_init(const Args& a, hipStream_t st);
// round r = 1, 2, ...: exit[r & 1] = F(entry by exit[(r - 1) & 1]); flags[r & 1] is raised where an entry state changed, flags[(r + 1) & 1] cleared
hipError_t launch_sync_round(const Args& a, uint32_t r, hipStream_t st);
// after the last round r: the block-count scan and the last pass into a.coef; flags[2] gets the first error bit
hipError_t launch_write(const Args& a, uint32_t r, hipStream_t st);
// DC scan, inverse DCT into the planes, upsampling and colour conversion into a.out
hipError_t launch_pixels(const Args& a, hipStream_t st);

}  // namespace jpegdec

}  // namespace v1c
