// kernels_jpegxf.hip -- the lossless JPEG composer's kernel (v1c_jpeg_compose, jpegxf.hip): k_jxf_gather is the transcoder's gather
// (kernels_jpegxc.hip: k_jxc_gather) with a source file and a transform per region.  It copies the blocks of an output -- rectangles of
// the MCUs of up to four decoded files -- from the decoders' coefficient stores into the encoder's, the DC a value, and rotates, flips
// or transposes them on the way: MCUs within the region, luma blocks within the MCU and coefficients within the block change places,
// and the coefficients of odd frequency along a mirrored axis change sign (jpegxf_core.hpp).  No inverse DCT, no pixels, no forward
// DCT.  INTEGRATION.md section 10 has the contract, DESIGN.md section 20 the design.  A code object of its own: the codecs' and the
// transcoder's code objects do not change with it.
//
// As in k_jxc_gather a block is 128 bytes that eight lanes move as eight 16-byte words: one global_load_dwordx4 and one
// global_store_dwordx4 per lane, a wave's stores 1024 contiguous bytes.  The signs are a per-lane byte of the transform's 64-bit mask
// over the packed 16-bit words.  A transposing block goes through LDS: its eight lanes store their words as they came (128 bytes of the
// workgroup's 4 KB) and each reads the eight 16-bit coefficients of its word of the result from their transposed places.  The
// transform is uniform over the eight lanes of a block, not over a wave: lanes of untransposed blocks skip the LDS traffic.  Nothing
// waits on another workgroup and the region search is bounded by kMaxRegions.
#include <hip/hip_runtime.h>

#include "jpegxf_launch.hpp"

namespace v1c {
namespace jpegxf {

namespace {

// the 16-bit halves of w with those negated whose bit of `neg` is set (bit 0: the low half), and whether both are coefficients the
// encoder codes; lo_dc: the low half is the block's DC, already judged
__device__ __forceinline__ uint32_t signed_pair(uint32_t w, uint32_t neg, bool lo_dc, bool& ok)
{
    int lo = (int16_t)(w & 0xffffu), hi = (int16_t)(w >> 16);
    lo = (neg & 1u) ? -lo : lo;
    hi = (neg & 2u) ? -hi : hi;
    ok &= (lo_dc | jpegxc::codable(lo, false)) & jpegxc::codable(hi, false);
    return ((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16);
}

}  // namespace

// 32 blocks per workgroup, eight lanes each.  The sources and the region list come with the kernel's arguments: constant memory, read
// with scalar loads where the index is uniform.
__global__ __launch_bounds__(256) void k_jxf_gather(GatherArgs a)
{
    __shared__ uint4 lds[256];
    const uint32_t slot = threadIdx.x >> 3, part = threadIdx.x & 7u;
    const uint32_t b = blockIdx.x * 32u + slot;
    const bool live = b < a.dst_nblocks;
    const jpegdec::Geom& g0 = a.src[0].g;  // (every source has the components and sampling factors of the first: jpegxf_host.hpp)
    SourceBlock sb{0, 0, kNone};
    if (live)
        sb = source_block(a.regions, a.dst_mcux, g0.hs, g0.vs, g0.bpm, b);
    uint4 v = make_uint4(0u, 0u, 0u, 0u);  // (a block no region holds: the host refuses such an output before any launch)
    int dc = 0;                            // the DC as it is judged: before it is cut to the 16 bits stored
    const bool held = sb.block != kNone;
    if (held) {
        // (the source's index is per block, not per wave: its descriptor is picked by comparison, never by an indexed load of the arguments)
        const uint32_t s = sb.source;
        const int16_t* coef = s == 0 ? a.src[0].coef : s == 1 ? a.src[1].coef : s == 2 ? a.src[2].coef : a.src[3].coef;
        v = ((const uint4*)coef)[(size_t)sb.block * 8 + part];
        if (part == 0) {
            if (s == 0)
                dc = jpegxc::dc_value(a.src[0].g, a.src[0].dcoff, sb.block);
            else if (s == 1)
                dc = jpegxc::dc_value(a.src[1].g, a.src[1].dcoff, sb.block);
            else if (s == 2)
                dc = jpegxc::dc_value(a.src[2].g, a.src[2].dcoff, sb.block);
            else
                dc = jpegxc::dc_value(a.src[3].g, a.src[3].dcoff, sb.block);
        }
    }
    // the transposing blocks: their words through LDS, read back 16 bits at a time from the transposed places
    const bool transposing = held && (sb.code & kTranspose);
    if (transposing)
        lds[threadIdx.x] = v;
    __syncthreads();
    if (transposing) {
        const uint16_t* blk = (const uint16_t*)(lds + slot * 8u);
        const uint64_t from = transposed_from(part);
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t lo = blk[(uint32_t)(from >> (16 * k)) & 0x3fu], hi = blk[(uint32_t)(from >> (16 * k + 8)) & 0x3fu];
            w[k] = lo | hi << 16;
        }
        v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    const uint32_t neg = (uint32_t)(negated(sb.code) >> (8u * part)) & 0xffu;
    bool ok = true;
    if (part == 0) {
        ok = jpegxc::codable(dc, true);
        v.x = (v.x & 0xffff0000u) | (uint32_t)(uint16_t)dc;
    }
    v.x = signed_pair(v.x, neg, part == 0, ok);
    v.y = signed_pair(v.y, neg >> 2, false, ok);
    v.z = signed_pair(v.z, neg >> 4, false, ok);
    v.w = signed_pair(v.w, neg >> 6, false, ok);
    if (live) {
        ((uint4*)a.dst)[(size_t)b * 8 + part] = v;
        if (!ok)
            atomicOr(a.flag, 1u);
    }
}

hipError_t launch_gather(const GatherArgs& a, hipStream_t st)
{
    hipLaunchKernelGGL(k_jxf_gather, dim3((a.dst_nblocks + 31) / 32), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace jpegxf
}  // namespace v1c
