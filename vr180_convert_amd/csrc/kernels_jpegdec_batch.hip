// kernels_jpegdec_batch.hip -- the device JPEG decoder's kernels for a batch of files (v1c_jpeg_decode_batch): the eight kernels of
// kernels_jpegdec.hip over a flat work list.  A workgroup finds its file by a bounded binary search over the first workgroups of the
// files (file_of, jpegdec_batch.hpp), takes that file's Args from a device array and does what the single-file kernel's workgroup of the
// same index within the file does: both call the same body of jpegdec_kernels.hpp.  The file is uniform per workgroup, so the Huffman
// tables are staged in LDS once per workgroup as there.  DESIGN.md section 15 has the design.
//
// Nothing waits on another workgroup; every loop is bounded (the bodies' loops, and the file search by 32 halvings).  A file rests
// from the round after its first quiet one (file_active): its workgroups return before they touch a table or a state.
#include <hip/hip_runtime.h>

#include "jpegdec_kernels.hpp"

namespace v1c {
namespace jpegdec {

namespace {

// the workgroup's file and, through wg, its index within the file
__device__ __forceinline__ const Args& file_args(const Batch& b, int list, uint32_t& wg)
{
    const uint32_t* first = b.first + (size_t)list * (b.n + 1);
    const uint32_t f = file_of(first, b.n, blockIdx.x);
    wg = blockIdx.x - first[f];
    return b.args[f];
}

}  // namespace

__global__ __launch_bounds__(256) void k_jdecb_count(Batch b)
{
    uint32_t wg;
    const Args& a = file_args(b, kByPiece, wg);
    count_body(a, wg);
}

__global__ __launch_bounds__(256) void k_jdecb_place(Batch b)
{
    uint32_t wg;
    const Args& a = file_args(b, kByPiece, wg);
    place_body(a, wg);
}

__global__ __launch_bounds__(256) void k_jdecb_init(Batch b)
{
    uint32_t wg;
    const Args& a = file_args(b, kBySub, wg);
    init_body(a, wg);
}

// One round of every file that is still moving.  Round r raises slot r % 3 of the file's flags, clears slot (r + 1) % 3 and reads slot
// (r - 1) % 3, which no workgroup of this launch writes.  A resting file's first workgroup passes the zero on, so the file rests in
// every later round as well, and the host reads a quiet round for it.
__global__ __launch_bounds__(256) void k_jdecb_sync(Batch b, uint32_t r)
{
    __shared__ Table t[8];
    uint32_t wg;
    const Args& a = file_args(b, kBySub, wg);
    if (!file_active(a.flags, r, a.nsub)) {
        if (wg == 0 && threadIdx.x == 0)
            a.flags[r % kRoundSlots] = 0;
        return;
    }
    load_tables(t, a.tab, threadIdx.x);
    __syncthreads();
    sync_body(a, wg, r, t, &a.flags[r % kRoundSlots], &a.flags[(r + 1) % kRoundSlots]);
}

// the last pass of every file, by the file's own last round
__global__ __launch_bounds__(256) void k_jdecb_write(Batch b)
{
    __shared__ Table t[8];
    uint32_t wg;
    const Args& a = file_args(b, kBySub, wg);
    const uint32_t r = b.rounds[(uint32_t)(&a - b.args)];
    load_tables(t, a.tab, threadIdx.x);
    __syncthreads();
    write_body(a, wg, r, t, &a.flags[kErrSlot]);
}

// The pixel stage.  A file the last pass found damaged has none: its workgroups return (uniformly, in front of any barrier), so that
// the work lists can be uploaded once, before the verdict is known.
__global__ __launch_bounds__(256) void k_jdecb_dcgather(Batch b)
{
    uint32_t wg;
    const Args& a = file_args(b, kByBlock, wg);
    if (a.flags[kErrSlot] != kNoError)
        return;
    dcgather_body(a, wg);
}

__global__ __launch_bounds__(256) void k_jdecb_idct(Batch b)
{
    __shared__ int tile[32][8][9];
    __shared__ __attribute__((aligned(16))) int16_t zz[32 * 64];
    __shared__ uint16_t q[4][64];
    uint32_t wg;
    const Args& a = file_args(b, kByTile, wg);
    if (a.flags[kErrSlot] != kNoError)
        return;
    idct_body(a, wg, tile, zz, q);
}

__global__ __launch_bounds__(256) void k_jdecb_colour(Batch b)
{
    uint32_t wg;
    const Args& a = file_args(b, kByPixel, wg);
    if (a.flags[kErrSlot] != kNoError)
        return;
    colour_body(a, wg);
}

namespace {

// the grid of a list; 0 where it is empty
uint32_t total(const Batch& b, const BatchHost& h, int list)
{
    return h.first[(size_t)list * (b.n + 1) + b.n];
}

}  // namespace

#define V1C_LAUNCH_LIST(kernel, list, ...)                                                           \
    do {                                                                                             \
        if (const uint32_t grid = total(b, h, list))                                                 \
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, st, b, ##__VA_ARGS__);              \
    } while (0)

hipError_t launch_unstuff_batch(const Batch& b, const BatchHost& h, hipStream_t st)
{
    V1C_LAUNCH_LIST(k_jdecb_count, kByPiece);
    for (uint32_t f = 0; f < b.n; f++) {
        const Args& a = h.args[f];
        const hipError_t e = jpeg::launch_scan(a.drop, a.pieces, a.sums, a.dropoff, st);
        if (e != hipSuccess)
            return e;
    }
    V1C_LAUNCH_LIST(k_jdecb_place, kByPiece);
    return hipGetLastError();
}

hipError_t launch_sync_init_batch(const Batch& b, const BatchHost& h, hipStream_t st)
{
    V1C_LAUNCH_LIST(k_jdecb_init, kBySub);
    return hipGetLastError();
}

hipError_t launch_sync_round_batch(const Batch& b, const BatchHost& h, uint32_t r, hipStream_t st)
{
    V1C_LAUNCH_LIST(k_jdecb_sync, kBySub, r);
    return hipGetLastError();
}

hipError_t launch_write_batch(const Batch& b, const BatchHost& h, hipStream_t st)
{
    for (uint32_t f = 0; f < b.n; f++) {
        const Args& a = h.args[f];
        const hipError_t e = jpeg::launch_scan(a.count, a.nsub, a.sums, a.first, st);
        if (e != hipSuccess)
            return e;
    }
    V1C_LAUNCH_LIST(k_jdecb_write, kBySub);
    return hipGetLastError();
}

hipError_t launch_pixels_batch(const Batch& b, const BatchHost& h, hipStream_t st)
{
    V1C_LAUNCH_LIST(k_jdecb_dcgather, kByBlock);
    for (uint32_t f = 0; f < b.n; f++) {
        if (h.skip[f])
            continue;
        const Args& a = h.args[f];
        const hipError_t e = jpeg::launch_scan(a.dcd, a.g.nblocks, a.sums, a.dcoff, st);
        if (e != hipSuccess)
            return e;
    }
    V1C_LAUNCH_LIST(k_jdecb_idct, kByTile);
    V1C_LAUNCH_LIST(k_jdecb_colour, kByPixel);
    return hipGetLastError();
}

#undef V1C_LAUNCH_LIST

}  // namespace jpegdec
}  // namespace v1c
