// jpeg_chunk.hpp -- where the pieces of an encoder chunk lie in its workspace, and the end of a chunk on the host: the layout of the
// stages' buffers and of the head in front of them, the kernels' arguments over both, and the read-back of the sizes, the check, the
// copies of the scans and the tables' records with their two synchronisations.  Shared by the batch encoder (jpeg.hip) and the
// lossless entries (jpegx_chain.hpp), which put a chunk behind their decoders' buffers in one allocation.  Host code only: the structs
// it fills are the kernels' (jpeg_launch.hpp, jpeg_batch.hpp, jpeg_opt_kernels.hpp), nothing here is launched.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <vector>

#include "host_util.hpp"
#include "jpeg_batch.hpp"
#include "jpeg_opt_kernels.hpp"

namespace v1c {
namespace jpeg {

// The stages' buffers for `t` entries back to back behind the `head` bytes the caller lays out itself, each aligned to 256 bytes.
struct StageLayout {
    size_t o_coef, o_bits, o_bitoff, o_ibytes, o_ioff, o_raw, o_ffcnt, o_ffoff, o_sums, o_out;
    size_t raw_bytes;  // of buf.raw, to be zeroed
    size_t bytes;      // of the workspace, head included

    Buffers at(uint8_t* base) const
    {
        Buffers buf;
        buf.coef = (int16_t*)(base + o_coef), buf.bits = (uint32_t*)(base + o_bits), buf.bitoff = (uint64_t*)(base + o_bitoff);
        buf.ibytes = (uint32_t*)(base + o_ibytes), buf.ioff = (uint64_t*)(base + o_ioff), buf.raw = (uint32_t*)(base + o_raw);
        buf.ffcnt = (uint32_t*)(base + o_ffcnt), buf.ffoff = (uint64_t*)(base + o_ffoff), buf.sums = (uint64_t*)(base + o_sums);
        buf.out = base + o_out;
        return buf;
    }
};

inline StageLayout stage_layout(size_t head, const Totals& t)
{
    StageLayout s{};
    s.raw_bytes = align256(t.pieces * kPiece + 16);
    s.o_coef = head, s.o_bits = s.o_coef + align256(t.nblocks * 128), s.o_bitoff = s.o_bits + align256(t.nblocks * 4);
    s.o_ibytes = s.o_bitoff + align256((t.nblocks + 1) * 8), s.o_ioff = s.o_ibytes + align256(t.nint * 4);
    s.o_raw = s.o_ioff + align256((t.nint + 1) * 8), s.o_ffcnt = s.o_raw + s.raw_bytes, s.o_ffoff = s.o_ffcnt + align256(t.pieces * 4);
    s.o_sums = s.o_ffoff + align256((t.pieces + 1) * 8), s.o_out = s.o_sums + align256(sums_of(t, kScanChunk) * 8);
    s.bytes = s.o_out + align256(t.out_bytes + 8);
    return s;
}

// The head of a chunk of n images with ntabs Tables and nslots optimising images.  Uploaded in one copy, [0, o_sizes): descriptors,
// work lists, Tables, and for an optimising chunk every image's slot and the slots.  Read back in one copy, back_bytes from o_sizes:
// the sizes, then the records.  Zeroed with them, zero_bytes from o_sizes: the histograms, and the 256 bytes behind them that a caller
// with `flag` asks for -- the lossless entries' gathers raise a word there.
struct HeadLayout {
    size_t o_im, o_first, o_tabs, o_slotof, o_slots, o_sizes, o_rec, o_hist, o_flag;
    size_t bytes, back_bytes, zero_bytes;
};

inline HeadLayout head_layout(uint32_t n, size_t ntabs, size_t nslots, bool flag)
{
    HeadLayout h{};
    h.o_im = 0, h.o_first = h.o_im + align256((size_t)n * sizeof(Image)), h.o_tabs = h.o_first + align256((size_t)kWorkLists * (n + 1) * 4);
    h.o_slotof = h.o_tabs + align256(ntabs * sizeof(Tables));
    h.o_slots = h.o_slotof + (nslots ? align256((size_t)n * 4) : 0), h.o_sizes = h.o_slots + align256(nslots * sizeof(OptSlot));
    h.o_rec = h.o_sizes + align256((size_t)n * 8), h.o_hist = h.o_rec + align256(nslots * sizeof(DhtRecord));
    h.o_flag = h.o_hist + align256(nslots * sizeof(Hist));
    h.bytes = h.o_flag + (flag ? 256 : 0);
    h.back_bytes = nslots ? h.o_rec + nslots * sizeof(DhtRecord) - h.o_sizes : (size_t)n * 8;
    h.zero_bytes = nslots || flag ? h.bytes - h.o_sizes : (size_t)n * 8;
    return h;
}

// the optimising images' part of the host's copy `up` of the head; slot_of: per image its slot, or -1
inline void stage_slots(uint8_t* up, const HeadLayout& h, const std::vector<int32_t>& slot_of, const std::vector<OptSlot>& slots)
{
    if (slots.empty())
        return;
    std::memcpy(up + h.o_slotof, slot_of.data(), slot_of.size() * 4);
    std::memcpy(up + h.o_slots, slots.data(), slots.size() * sizeof(OptSlot));
}

// the kernels' arguments of a chunk whose head lies at `base` (device address) and whose buffers are buf
inline void chunk_args(const HeadLayout& h, uint8_t* base, uint32_t n, size_t nslots, const Totals& t, const Buffers& buf, Batch& b, OptBatch& o)
{
    b = Batch{};
    b.im = (const Image*)(base + h.o_im), b.first = (const uint32_t*)(base + h.o_first), b.tabs = (const Tables*)(base + h.o_tabs);
    b.n = n, b.t = t;
    b.sizes = (uint64_t*)(base + h.o_sizes);
    b.buf = buf;
    o = OptBatch{};
    o.slot_of = (const int32_t*)(base + h.o_slotof), o.slots = (const OptSlot*)(base + h.o_slots), o.nslots = (uint32_t)nslots;
    o.hist = (Hist*)(base + h.o_hist), o.rec = (DhtRecord*)(base + h.o_rec), o.tabs = (Tables*)(base + h.o_tabs);
}

// where the results of one image go: the caller's fields
struct Result {
    uint8_t* out_host;
    uint64_t* size;
    uint8_t* dht;        // optimising images: V1C_JPEG_DHT_MAX bytes for the DHT segment's body
    uint32_t* dht_size;
};

// the step of finish_chunk that failed
enum FinishStep { kFinished = 0, kFinishKernels, kFinishSizes, kFinishCopy };

// The end of a chunk whose kernels are queued (e: what queuing them and everything in front of them gave): all sizes and, in the same
// copy, the records of the optimising images' tables, and synchronisation 1 -- on an error too, so that nothing reads the host's
// buffers behind it --; the check of every size against the image's bound; every image's scan to its out_host, and synchronisation 2;
// then the sizes and the tables into the caller's fields, to(f) of image f.  im, slot_of: the host's copies.  kFinished, or the step
// that failed with its error in e (kFinishSizes: hipErrorUnknown).
template <class To>
inline FinishStep finish_chunk(const Batch& b, const HeadLayout& h, const Image* im, const std::vector<int32_t>& slot_of, To to, hipStream_t st,
                               hipError_t& e)
{
    std::vector<uint8_t> back(h.back_bytes, 0);
    if (e == hipSuccess)
        e = hipMemcpyAsync(back.data(), b.sizes, h.back_bytes, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);  // 1: the sizes and the records
    if (e == hipSuccess)
        e = es;
    if (e != hipSuccess)
        return kFinishKernels;
    const uint64_t* sizes = (const uint64_t*)back.data();
    for (uint32_t f = 0; f < b.n; f++)
        if (sizes[f] == 0 || sizes[f] > scan_bound(im[f].g))
            return e = hipErrorUnknown, kFinishSizes;
    for (uint32_t f = 0; f < b.n && e == hipSuccess; f++)
        e = hipMemcpyAsync(to(f).out_host, b.buf.out + im[f].out0, sizes[f], hipMemcpyDeviceToHost, st);
    const hipError_t ec = hipStreamSynchronize(st);  // 2: the scans
    if (e == hipSuccess)
        e = ec;
    if (e != hipSuccess)
        return kFinishCopy;
    for (uint32_t f = 0; f < b.n; f++) {
        const Result r = to(f);
        *r.size = sizes[f];
        if (slot_of[f] >= 0)
            *r.dht_size = dht_body(((const DhtRecord*)(back.data() + (h.o_rec - h.o_sizes)))[slot_of[f]], r.dht);
    }
    return kFinished;
}

}  // namespace jpeg
}  // namespace v1c
