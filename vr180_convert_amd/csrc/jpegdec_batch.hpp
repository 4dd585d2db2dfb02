// jpegdec_batch.hpp -- what the batched JPEG decoder (v1c_jpeg_decode_batch: jpegdec.hip, kernels_jpegdec_batch.hip) adds to the
// single-file one, and nothing of the arithmetic: the work list that maps a workgroup to its file, the per-file flag words with the rule that lets a
// converged file rest, and the cut of a list of files into chunks under a workspace budget.  DESIGN.md section 15.
//
// __host__ __device__ / plain C++ so that tests/host_jpegdec_batch/ runs exactly this code in its sequential copy of the kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace v1c {
namespace jpegdec {

// The work lists of a chunk of n files, one per grid shape: first[list * (n + 1) + f] is the first workgroup of file f in that list's
// kernels, [.. + n] their number.
enum WorkList { kByPiece = 0, kBySub = 1, kByBlock = 2, kByTile = 3, kByPixel = 4, kWorkLists = 5 };

// The file of workgroup wg < first[n]: the last f with first[f] <= wg, which is never one of an empty range.  Bounded by 32 halvings.
__host__ __device__ inline uint32_t file_of(const uint32_t* first, uint32_t n, uint32_t wg)
{
    uint32_t lo = 0, hi = n - 1;
    for (int it = 0; it < 32 && lo < hi; it++) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (first[mid] <= wg)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// Every file of a chunk has kFlagWords words, all files' back to back so that one copy brings them to the host: three round flags in
// rotation and the last pass's first error bit.  Round r raises slot r % 3 where an entry state of the file changed, clears slot
// (r + 1) % 3 and READS slot (r - 1) % 3, which no workgroup of round r writes -- with the single-file call's two slots the slot read
// would be the slot cleared.  A file whose previous round raised nothing rests: its first workgroup only passes the zero on to slot
// r % 3, so the file rests in every later round too and its exit buffers, counts and parity stay what its last active round left.
constexpr uint32_t kRoundSlots = 3, kErrSlot = 3, kFlagWords = 4;

__host__ __device__ inline bool file_active(const uint32_t* flags, uint32_t r, uint32_t nsub)
{
    return r == 1 || (r <= nsub + 1 && flags[(r - 1) % kRoundSlots] != 0);  // (nsub + 1: the single-file call's bound on its rounds)
}

// The chunks of a batch: files in order while the sum of their workspaces stays within `budget` and no work list passes 2^31 - 1
// workgroups; a file larger than the budget is a chunk of its own.  Returns the end (one past the last file) of every chunk.
// groups[f]: the largest number of workgroups file f has in any list.
constexpr uint64_t kDefaultBatchWorkspace = (uint64_t)1 << 30;

inline std::vector<uint32_t> chunk_ends(const std::vector<uint64_t>& bytes, const std::vector<uint64_t>& groups, uint64_t budget)
{
    std::vector<uint32_t> ends;
    uint64_t sum = 0, wg = 0;
    uint32_t start = 0;
    for (uint32_t f = 0; f < bytes.size(); f++) {
        if (f > start && (sum + bytes[f] > budget || wg + groups[f] > 0x7fffffffu)) {
            ends.push_back(f);
            start = f, sum = wg = 0;
        }
        sum += bytes[f], wg += groups[f];
    }
    if (!bytes.empty())
        ends.push_back((uint32_t)bytes.size());
    return ends;
}

}  // namespace jpegdec
}  // namespace v1c
