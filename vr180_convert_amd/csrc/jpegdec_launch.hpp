// jpegdec_launch.hpp -- launchers of the JPEG decoder's kernels (kernels_jpegdec.hip), called by the C ABI in jpegdec.hip, and the
// host's step from one file's upload to its coefficients (decode_to_coef), which the lossless entries (jpegx_chain.hpp) run too.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "host_util.hpp"
#include "jpeg_launch.hpp"
#include "jpegdec_batch.hpp"
#include "jpegdec_core.hpp"
#include "jpegdec_host.hpp"

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

// Where the buffers of one file lie: what is uploaded (tables, segment offsets, first subsequences, the scan) back to back from the
// upload's base, and what the kernels make back to back from the work's base, each piece aligned to 256 bytes.  The single call puts
// the work behind the upload in one allocation; a batch puts all its files' uploads in front of all their work, so that one copy
// brings a chunk's files to the device.
struct Layout {
    size_t o_tab, o_segoff, o_subfirst, o_scan, up_bytes;                                // from the upload's base
    size_t o_flags, o_drop, o_dropoff, o_u, u_bytes, o_exit0, o_exit1, o_last, o_count;  // from the work's base
    size_t o_first, o_coef, coef_bytes, o_dcd, o_dcoff, o_sums, o_p0, p0_bytes, pc_bytes, work_bytes;
    size_t bytes;                                                                        // up_bytes + work_bytes
    uint32_t pieces;
};

inline Layout layout_of(const Parsed& ps, uint32_t nsub)
{
    const Geom& g = ps.g;
    const size_t nseg = g.nseg;
    Layout l{};
    l.pieces = ((uint32_t)ps.scan_len + kPiece - 1) / kPiece;
    const size_t pieces = l.pieces, nu = ps.segoff.back();
    l.o_tab = 0, l.o_segoff = l.o_tab + align256(sizeof(Tables)), l.o_subfirst = l.o_segoff + align256((nseg + 1) * 4);
    l.o_scan = l.o_subfirst + align256((nseg + 1) * 4), l.up_bytes = l.o_scan + align256((pieces + 1) * kPiece);
    const uint64_t nmax = pieces > nsub ? (pieces > g.nblocks ? pieces : g.nblocks) : (nsub > g.nblocks ? nsub : g.nblocks);
    l.o_flags = 0, l.o_drop = l.o_flags + 256, l.o_dropoff = l.o_drop + align256(pieces * 4);
    l.o_u = l.o_dropoff + align256((pieces + 1) * 8), l.u_bytes = align256(nu + 16);
    l.o_exit0 = l.o_u + l.u_bytes, l.o_exit1 = l.o_exit0 + align256((size_t)nsub * 8), l.o_last = l.o_exit1 + align256((size_t)nsub * 8);
    l.o_count = l.o_last + align256((size_t)nsub * 8), l.o_first = l.o_count + align256((size_t)nsub * 4);
    l.o_coef = l.o_first + align256(((size_t)nsub + 1) * 8), l.coef_bytes = align256((size_t)g.nblocks * 128);
    l.o_dcd = l.o_coef + l.coef_bytes, l.o_dcoff = l.o_dcd + align256((size_t)g.nblocks * 4);
    l.o_sums = l.o_dcoff + align256(((size_t)g.nblocks + 1) * 8);
    l.o_p0 = l.o_sums + align256((nmax / jpeg::kScanChunk + 2) * 8);
    l.p0_bytes = align256((size_t)plane_pitch(g, 0) * plane_rows(g, 0)), l.pc_bytes = align256((size_t)plane_pitch(g, 1) * plane_rows(g, 1));
    l.work_bytes = l.o_p0 + l.p0_bytes + (g.nc == 3 ? 2 * l.pc_bytes : 0);
    l.bytes = l.up_bytes + l.work_bytes;
    return l;
}

// the Args of a file whose upload lies at `up` and whose work at `work` (device addresses); flags: the file's flag words
inline Args args_of(const Parsed& ps, const Layout& l, uint32_t nsub, uint32_t S, uint8_t* up, uint8_t* work, uint32_t* flags, void* out,
                    int64_t pitch, int out_cn)
{
    const Geom& g = ps.g;
    Args a{};
    a.g = g;
    a.tab = (const Tables*)(up + l.o_tab);
    a.scan = up + l.o_scan;
    a.scan_len = (uint32_t)ps.scan_len, a.pieces = l.pieces;
    a.drop = (uint32_t*)(work + l.o_drop);
    a.dropoff = (uint64_t*)(work + l.o_dropoff);
    a.u = (uint32_t*)(work + l.o_u);
    a.segoff = (const uint32_t*)(up + l.o_segoff);
    a.subfirst = (const uint32_t*)(up + l.o_subfirst);
    a.nsub = nsub, a.S = S;
    a.exit[0] = (State*)(work + l.o_exit0), a.exit[1] = (State*)(work + l.o_exit1);
    a.last = (State*)(work + l.o_last);
    a.count = (uint32_t*)(work + l.o_count);
    a.first = (uint64_t*)(work + l.o_first);
    a.flags = flags;
    a.coef = (int16_t*)(work + l.o_coef);
    a.dcd = (uint32_t*)(work + l.o_dcd);
    a.dcoff = (uint64_t*)(work + l.o_dcoff);
    a.sums = (uint64_t*)(work + l.o_sums);
    a.plane[0] = work + l.o_p0;
    a.plane[1] = g.nc == 3 ? work + l.o_p0 + l.p0_bytes : nullptr;
    a.plane[2] = g.nc == 3 ? work + l.o_p0 + l.p0_bytes + l.pc_bytes : nullptr;
    a.out = (uint8_t*)out, a.pitch = pitch, a.out_cn = (uint32_t)out_cn;
    return a;
}

// a file's upload in host memory at `stage` (zeroed by the caller): tables, segment offsets, first subsequences, the scan
inline void stage_file(uint8_t* stage, const Parsed& ps, const Layout& l, const std::vector<uint32_t>& subfirst, const uint8_t* file)
{
    const size_t nseg = ps.g.nseg;
    std::memcpy(stage + l.o_tab, &ps.tab, sizeof(Tables));
    std::memcpy(stage + l.o_segoff, ps.segoff.data(), (nseg + 1) * 4);
    std::memcpy(stage + l.o_subfirst, subfirst.data(), (nseg + 1) * 4);
    std::memcpy(stage + l.o_scan, file + ps.scan_start, (size_t)ps.scan_len + 2);  // (the parse saw the two bytes of the marker behind the scan)
}

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

// One file from its staged upload to its coefficients, for every entry that decodes one file at a time (v1c_jpeg_decode, and the
// lossless entries source by source): the upload from `stage` (host memory, l.up_bytes; a's upload lies at a.tab), the zeroing of the
// flags, the error word, a.u and a.coef, the unstuffing, and the rounds -- at most nsub + 1, since round r fixes the first r entry
// states of every segment for good -- with the last pass behind them.  The host reads a flag between the rounds: *more (host memory)
// receives it, and the stream is SYNCHRONISED once per round; the last pass is queued, not waited for.  `stage` and `more` must stay
// alive until the caller's next synchronisation.  Returns the first error, and the rounds in *rounds whatever happened.
inline hipError_t decode_to_coef(const Args& a, const Layout& l, const uint8_t* stage, uint32_t nsub, hipStream_t st, volatile uint32_t* more,
                                 uint32_t* rounds)
{
    hipError_t e = hipMemcpyAsync((uint8_t*)a.tab - l.o_tab, stage, l.up_bytes, hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = hipMemsetAsync(a.flags, 0, 8, st);
    if (e == hipSuccess)
        e = hipMemsetAsync(a.flags + 2, 0xff, 4, st);  // kNoError
    if (e == hipSuccess)
        e = hipMemsetAsync(a.u, 0, l.u_bytes, st);
    if (e == hipSuccess)
        e = hipMemsetAsync(a.coef, 0, l.coef_bytes, st);
    if (e == hipSuccess)
        e = launch_unstuff(a, st);
    if (e == hipSuccess)
        e = launch_sync_init(a, st);
    uint32_t r = 0;
    while (e == hipSuccess) {
        r++;
        e = launch_sync_round(a, r, st);
        if (e == hipSuccess)
            e = hipMemcpyAsync((void*)more, a.flags + (r & 1u), 4, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess)
            e = hipStreamSynchronize(st);
        if (e != hipSuccess || *more == 0 || r > nsub)
            break;
    }
    *rounds = r;
    return e == hipSuccess ? launch_write(a, r, st) : e;
}

// ---- a batch: a chunk of n files in shared launches (kernels_jpegdec_batch.hip) --------------------------------
struct Batch {
    const Args* args;        // n, on the device; every file's flags are kFlagWords words (jpegdec_batch.hpp)
    const uint32_t* first;   // kWorkLists x (n + 1): the work lists
    const uint32_t* rounds;  // n: every file's last round, whose parity the last pass reads the exit states by
    uint32_t n;
};

// What the host knows of the chunk's files, for the grids and for the scans, which stay one set of launches per file: they lie outside
// the round loop, and nothing synchronises between them.
struct BatchHost {
    const Args* args;       // n, on the host
    const uint32_t* first;  // kWorkLists x (n + 1), on the host: what b.first holds when the launch runs
    const int* skip;        // n: nonzero for a file without the pixel stage
};

hipError_t launch_unstuff_batch(const Batch& b, const BatchHost& h, hipStream_t st);
hipError_t launch_sync_init_batch(const Batch& b, const BatchHost& h, hipStream_t st);
// round r of every file that is still moving: one launch
hipError_t launch_sync_round_batch(const Batch& b, const BatchHost& h, uint32_t r, hipStream_t st);
// the block-count scans and the last pass; b.rounds must have arrived
hipError_t launch_write_batch(const Batch& b, const BatchHost& h, hipStream_t st);
// the pixel stage; the workgroups of a file whose flags hold an error bit return at once, and h.skip spares it the DC scan
hipError_t launch_pixels_batch(const Batch& b, const BatchHost& h, hipStream_t st);

}  // namespace jpegdec

}  // namespace v1c
