// jpegprog_core.hpp -- per-lane arithmetic of the device decoder of PROGRESSIVE JPEG files (kernels_jpegprog.hip, jpegdec.hip:
// v1c_jpeg_prog_decode): the geometry of one scan, the map from a scan's blocks to the file's MCU-major coefficient store, the step
// functions of the four scan kinds (ISO/IEC 10918-1 G.1.2: DC first, DC refinement, AC first, AC refinement), F_i over one subsequence
// and the last pass.  It sits on jpegdec_core.hpp -- the bit reader, the tables, the Geom -- and changes nothing there.
//
// __host__ __device__, and written per lane over plain pointers, so that tests/host_jpegdec_prog/jpegprog_emul.hip runs exactly this
// code on the host against the restatement (tests/jpgprog_ref.py).  INTEGRATION.md section 8 ("Progressive files") has the contract,
// DESIGN.md section 18 the design.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jpegdec_core.hpp"

namespace v1c {
namespace jpegprog {

using jpegdec::find_code;
using jpegdec::Geom;
using jpegdec::peek32;
using jpegdec::Table;
using jpegdec::Tables;

constexpr uint32_t kNoError = 0xffffffffu;
constexpr uint32_t kCountCap = 0x40000000u;  // a lane's block count saturates here (only garbage gets there)

enum Kind : uint32_t { kDCFirst = 0, kDCRefine = 1, kACFirst = 2, kACRefine = 3 };

// One scan.  Its blocks ("units") are numbered in the order the scan codes them: MCU by MCU for an interleaved scan, the component's
// own ceil(wc / 8) x ceil(hc / 8) blocks in raster order for a scan of one component (NOT the MCU-padded grid).
struct Scan {
    uint32_t kind, ni;       // ni: one component, not interleaved
    uint32_t Ss, Se, Al;
    uint32_t bps;            // blocks of one of the scan's MCUs (ni: 1)
    uint32_t nmcu, nunits;   // the scan's MCUs and blocks
    uint32_t ibl, nseg;      // blocks of a full segment; segments
    uint32_t bw, comp0;      // ni: blocks in a row of the component; the component
    uint32_t dcsel;          // four bits per block j of the scan's MCU: its DC table
    uint32_t acsel;          // the AC table (AC scans have one component)
    uint32_t ksel;           // four bits per j: the block's place in the FILE's MCU
    uint32_t csel;           // four bits per j: its number among its component's blocks of the MCU | the component's place in the scan << 2
    uint32_t nbsel, presel;  // four bits per component of the scan: its blocks in an MCU; those of the components in front of it
};

// the block of the file's store that unit u of the scan is
__host__ __device__ inline uint32_t block_of(const Geom& g, const Scan& sc, uint32_t u)
{
    if (sc.ni) {
        const uint32_t by = u / sc.bw, bx = u - by * sc.bw;
        if (sc.comp0 == 0) {
            const uint32_t my = by / g.vs, mx = bx / g.hs;
            return (my * g.mcux + mx) * g.bpm + (by - my * g.vs) * g.hs + (bx - mx * g.hs);
        }
        return (by * g.mcux + bx) * g.bpm + g.ny + sc.comp0 - 1;
    }
    const uint32_t mcu = u / sc.bps, j = u - mcu * sc.bps;
    return mcu * g.bpm + ((sc.ksel >> (4 * j)) & 15u);
}

// where the DC difference of unit u lies in the order the DC scan runs over (component by component), and where its segment's first
// unit of the same component does
__host__ __device__ inline void dd_pos(const Scan& sc, uint32_t u, uint32_t& pos, uint32_t& pos0)
{
    const uint32_t u0 = u / sc.ibl * sc.ibl;
    if (sc.ni) {
        pos = u, pos0 = u0;
        return;
    }
    const uint32_t mcu = u / sc.bps, j = u - mcu * sc.bps, m0 = u0 / sc.bps;
    const uint32_t cs = (sc.csel >> (4 * j)) & 15u, ci = cs >> 2, jc = cs & 3u;
    const uint32_t nb = (sc.nbsel >> (4 * ci)) & 15u, pre = (sc.presel >> (4 * ci)) & 15u;
    pos = sc.nmcu * pre + mcu * nb + jc, pos0 = sc.nmcu * pre + m0 * nb;
}

// State of the decoder between two steps.  run and b are those of an AC refinement scan, 0 in the others: there the bits a block takes
// depend on which of its coefficients earlier scans left nonzero, so the block belongs to the state.
struct PState {
    uint32_t p;    // bit of the next step in the unstuffed scan
    uint32_t zc;   // z | c << 8: zigzag index of the next coefficient (within the band), block within the scan's MCU
    uint32_t run;  // blocks of an end-of-band run still to end, the current one among them
    uint32_t b;    // the unit the state is in
};

__host__ __device__ inline bool operator==(const PState& a, const PState& b)
{
    return a.p == b.p && a.zc == b.zc && a.run == b.run && a.b == b.b;
}

// what one lane works on: a scan of a file
struct ScanArgs {
    Geom g;
    Scan sc;
    const Tables* tab;         // the tables in force at the scan
    const uint32_t* u;         // the unstuffed scan in whole words, two of them behind its last byte
    const uint32_t* segoff;    // nseg + 1
    const uint32_t* subfirst;  // nseg + 1
    uint32_t nsub, S;
    PState* exit[2];
    PState* last;
    uint32_t* count;
    uint64_t* first;           // nsub + 1: the exclusive scan of count
    uint32_t* flags;           // [0], [1]: a round's flag by its parity; [2]: the last pass's first error bit
    int16_t* coef;             // the file's store: nblocks x 64, zigzag, MCU-major
    uint32_t* dd;              // DC first: the differences ordered by component; after the last scan: the DC values by block
    uint64_t* ddoff;           // nunits + 1: their exclusive scan
    uint64_t* sums;            // the scans' per-chunk sums
};

struct Sub {
    uint32_t k, start, end, E;
    bool first, last;
};

__host__ __device__ inline Sub sub_of(const ScanArgs& a, uint32_t i)
{
    uint32_t lo = 0, hi = a.sc.nseg - 1;
    for (int it = 0; it < 32 && lo < hi; it++) {  // the last k with subfirst[k] <= i
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (a.subfirst[mid] <= i)
            lo = mid;
        else
            hi = mid - 1;
    }
    Sub s;
    s.k = lo;
    s.E = 8 * a.segoff[lo + 1];
    const uint32_t j = i - a.subfirst[lo];
    s.start = 8 * a.segoff[lo] + j * a.S;
    s.end = s.start + a.S < s.E ? s.start + a.S : s.E;
    s.first = j == 0;
    s.last = i + 1 == a.subfirst[lo + 1];
    return s;
}

// the state a segment begins in
__host__ __device__ inline PState seg_entry(const Scan& sc, const Sub& s)
{
    return PState{s.start, sc.kind >= kACFirst ? sc.Ss : 0u, 0u, sc.kind == kACRefine ? s.k * sc.ibl : 0u};
}

__host__ __device__ inline uint32_t bit_at(const uint32_t* u, uint32_t p)
{
    return (__builtin_bswap32(u[p >> 5]) >> (31u - (p & 31u))) & 1u;
}

// bits [lo, hi) of a 64-bit mask, 0 <= lo, hi <= 64
__host__ __device__ inline uint64_t bits_from(uint32_t lo)
{
    return lo >= 64 ? 0ull : ~0ull << lo;
}

// which coefficients of the band a block holds nonzero: what an AC refinement scan's bits depend on
__host__ __device__ inline uint64_t band_mask(const int16_t* blk, uint32_t Ss, uint32_t Se)
{
    const uint4* q = (const uint4*)blk;  // (a block is 128 bytes, aligned)
    uint64_t m = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint4 v = q[i];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            m |= (uint64_t)((w[j] & 0xffffu) != 0) << (8 * i + 2 * j);
            m |= (uint64_t)((w[j] >> 16) != 0) << (8 * i + 2 * j + 1);
        }
    }
    return m & bits_from(Ss) & ~bits_from(Se + 1);
}

// the correction bits of the coefficients in nz (ascending), read from bit q on: libjpeg's decode_mcu_AC_refine
__host__ __device__ inline void correct(int16_t* blk, uint64_t nz, const uint32_t* u, uint32_t q, uint32_t Al)
{
    const int p1 = 1 << Al;
    for (int it = 0; it < 64 && nz; it++, q++) {
        const int k = __builtin_ctzll(nz);
        nz &= nz - 1;
        if (bit_at(u, q)) {
            const int c = blk[k];
            if ((c & p1) == 0)
                blk[k] = (int16_t)(c >= 0 ? c + p1 : c - p1);
        }
    }
}

// The steps that start in [s.p, end) of a segment that ends at bit E; s becomes the exit state.  Returns the blocks completed.
// One step is one Huffman symbol with its extra bits and, in an AC refinement scan, the correction bits that belong to it -- or one
// block's share of a running end-of-band run there: the correction bits of what is left of the block.  A DC refinement step is one bit.
// The rules that make speculative decoding deterministic are jpegdec_core.hpp's: bits that start no code consume one bit, a run past
// the band's end ends the block, a step that would pass E stops the decode at E; a size above 1 in a refinement scan counts as 1.
// WRITE: the last pass -- writes the blocks from unit b on while b < bq, and returns the bit of the first bad step through *err.
// Not WRITE: nothing is written, and b is the state's (AC refinement) or unused.  t: dc[4], ac[4] of the scan.
template <bool WRITE>
__host__ __device__ inline uint32_t span(const ScanArgs& a, const Table* t, PState& s, uint32_t end, uint32_t E, uint32_t b, uint32_t bq,
                                         uint32_t* err)
{
    const Scan& sc = a.sc;
    const uint32_t* u = a.u;
    uint32_t p = s.p, z = s.zc & 255u, c = s.zc >> 8, run = s.run, n = 0;
    if (!WRITE)
        b = s.b;
    if (sc.kind == kDCFirst) {
        while (p < end && (!WRITE || b < bq)) {
            const uint32_t w = peek32(u, p);
            const uint32_t e = find_code(t[(sc.dcsel >> (4 * c)) & 3u], w);
            if (e == 0) {
                if (WRITE) {
                    *err = p;
                    break;
                }
                p++;
                continue;
            }
            const uint32_t len = e >> 8, sz = e & 15u;
            if (p + len + sz > E) {
                if (WRITE)
                    *err = p;
                p = E;
                break;
            }
            if (WRITE) {
                int v = 0;
                if (sz) {
                    v = (int)((w << len) >> (32u - sz));
                    if (v < (1 << (sz - 1)))
                        v -= (1 << sz) - 1;
                }
                uint32_t pos, pos0;
                dd_pos(sc, b, pos, pos0);
                a.dd[pos] = (uint32_t)v;
            }
            p += len + sz;
            c = c + 1 == sc.bps ? 0u : c + 1;
            n++, b++;
        }
    } else if (sc.kind == kDCRefine) {
        if (!WRITE) {
            n = p < end ? end - p : 0u, p = p < end ? end : p;
        } else {
            while (p < end && b < bq) {
                if (bit_at(u, p)) {
                    int16_t* dc = a.coef + (size_t)block_of(a.g, sc, b) * 64;
                    *dc = (int16_t)(*dc | (1 << sc.Al));
                }
                p++, n++, b++;
            }
        }
    } else if (sc.kind == kACFirst) {
        const Table& ta = t[4 + (sc.acsel & 3u)];
        int16_t* blk = WRITE && b < bq ? a.coef + (size_t)block_of(a.g, sc, b) * 64 : nullptr;
        while (p < end && (!WRITE || b < bq)) {
            const uint32_t w = peek32(u, p);
            const uint32_t e = find_code(ta, w);
            if (e == 0) {
                if (WRITE) {
                    *err = p;
                    break;
                }
                p++;
                continue;
            }
            const uint32_t len = e >> 8, sym = e & 255u, sz = sym & 15u, rn = sym >> 4;
            const uint32_t extra = sz ? sz : rn < 15 ? rn : 0u;
            if (p + len + extra > E) {
                if (WRITE)
                    *err = p;
                p = E;
                break;
            }
            const uint32_t raw = extra ? (w << len) >> (32u - extra) : 0u;
            const uint32_t p0 = p;
            p += len + extra;
            bool done = false;
            uint32_t blocks = 1;
            if (sz == 0 && rn < 15) {  // EOBn: this block and 2^n + extra - 1 behind it
                blocks = (1u << rn) + raw;
                if (WRITE && blocks > bq - b) {
                    *err = p0;
                    break;
                }
                done = true;
            } else {
                z += sz ? rn : 16u;
                if (z > sc.Se) {
                    if (WRITE) {
                        *err = p0;
                        break;
                    }
                    done = true;
                } else if (sz) {
                    if (WRITE) {
                        int v = (int)raw;
                        if (v < (1 << (sz - 1)))
                            v -= (1 << sz) - 1;
                        blk[z] = (int16_t)((uint32_t)v << sc.Al);
                    }
                    z++;
                    done = z > sc.Se;
                }
            }
            if (done) {
                z = sc.Ss;
                n = n + blocks > kCountCap ? kCountCap : n + blocks;
                b += blocks;
                if (WRITE && b < bq)
                    blk = a.coef + (size_t)block_of(a.g, sc, b) * 64;
            }
        }
    } else {
        const Table& ta = t[4 + (sc.acsel & 3u)];
        const uint32_t p1 = 1u << sc.Al;
        uint32_t mb = kNoError;  // the unit m and blk are of
        uint64_t m = 0;
        int16_t* blk = nullptr;
        // (a turn consumes a bit or a block of the run: bounded by the subsequence's bits and the 32767 blocks a run can have per symbol)
        while ((p < end || (end == E && run > 0)) && (!WRITE || b < bq)) {
            if (mb != b) {
                mb = b;
                blk = b < sc.nunits ? a.coef + (size_t)block_of(a.g, sc, b) * 64 : nullptr;
                m = blk ? band_mask(blk, sc.Ss, sc.Se) : 0ull;
            }
            if (run > 0) {  // one block's share of the run: the correction bits of what is left of it
                const uint64_t nz = m & bits_from(z);
                const uint32_t cnt = (uint32_t)__builtin_popcountll(nz);
                if (p + cnt > E) {
                    if (WRITE)
                        *err = p;
                    p = E;
                    break;
                }
                if (WRITE)
                    correct(blk, nz, u, p, sc.Al);
                p += cnt, run--, z = sc.Ss, n++, b++;
                continue;
            }
            const uint32_t w = peek32(u, p);
            const uint32_t e = find_code(ta, w);
            if (e == 0) {
                if (WRITE) {
                    *err = p;
                    break;
                }
                p++;
                continue;
            }
            const uint32_t len = e >> 8, sym = e & 255u, sz = sym & 15u, rn = sym >> 4;
            if (sz == 0 && rn < 15) {  // EOBn: the run begins with what is left of this block
                if (p + len + rn > E) {
                    if (WRITE)
                        *err = p;
                    p = E;
                    break;
                }
                run = (1u << rn) + (rn ? (w << len) >> (32u - rn) : 0u);
                p += len + rn;
                continue;
            }
            if (WRITE && sz > 1) {
                *err = p;
                break;
            }
            const uint32_t need = len + (sz ? 1u : 0u);
            // the (rn + 1)-th coefficient from z on that is still zero: where the new one goes, or where the run of 16 ends
            uint64_t zz = ~m & bits_from(z) & ~bits_from(sc.Se + 1);
            for (uint32_t i = 0; i < rn; i++)
                zz &= zz - 1;
            const uint32_t kz = zz ? (uint32_t)__builtin_ctzll(zz) : sc.Se + 1;
            const uint64_t nz = m & bits_from(z) & ~bits_from(kz);
            const uint32_t cnt = (uint32_t)__builtin_popcountll(nz);
            if (p + need + cnt > E) {
                if (WRITE)
                    *err = p;
                p = E;
                break;
            }
            if (WRITE) {
                if (kz > sc.Se) {
                    *err = p;
                    break;
                }
                correct(blk, nz, u, p + need, sc.Al);
                if (sz)
                    blk[kz] = (int16_t)((w >> (31u - len)) & 1u ? (int)p1 : -(int)p1);
            }
            p += need + cnt;
            z = kz + 1;
            if (z > sc.Se)
                z = sc.Ss, n++, b++;
        }
    }
    s.p = p, s.zc = z | c << 8, s.run = run, s.b = sc.kind == kACRefine ? b : 0u;
    return n;
}

// ---- what one lane of every kernel does (kernels_jpegprog.hip: lane = blockIdx.x * 256 + threadIdx.x; the host harness: a loop) ------

// before the first round: what F_i "gave" is the grid state of the subsequence behind it
__host__ __device__ inline void init_lane(const ScanArgs& a, uint32_t i)
{
    const Sub s = sub_of(a, i);
    PState x = seg_entry(a.sc, s);
    x.p = s.end, x.b = 0;
    a.exit[0][i] = x;
    a.last[i] = PState{kNoError, kNoError, kNoError, kNoError};
    a.count[i] = 0;
}

// one round; returns whether it changed the entry state of the subsequence behind
__host__ __device__ inline bool sync_lane(const ScanArgs& a, uint32_t i, uint32_t r, const Table* t)
{
    const PState* in = a.exit[(r - 1) & 1u];
    PState* out = a.exit[r & 1u];
    const Sub s = sub_of(a, i);
    const PState e = s.first ? seg_entry(a.sc, s) : in[i - 1];
    const PState was = in[i];
    if (e == a.last[i]) {
        out[i] = was;
        return false;
    }
    PState x = e;
    const uint32_t n = span<false>(a, t, x, s.end, s.E, 0, 0, nullptr);
    a.last[i] = e;
    a.count[i] = n;
    out[i] = x;
    return !s.last && !(x == was);
}

// the last pass; returns the first error bit or kNoError.  Only this pass judges the stream: a bad step, and a segment whose blocks are
// not the geometry's (a DC refinement segment: fewer bits than blocks -- its padding counts as steps).
__host__ __device__ inline uint32_t write_lane(const ScanArgs& a, uint32_t i, uint32_t r, const Table* t)
{
    const PState* fin = a.exit[r & 1u];
    const Sub s = sub_of(a, i);
    PState e = s.first ? seg_entry(a.sc, s) : fin[i - 1];
    const uint32_t i0 = a.subfirst[s.k], b0 = s.k * a.sc.ibl, bq = b0 + a.sc.ibl < a.sc.nunits ? b0 + a.sc.ibl : a.sc.nunits;
    const uint64_t done = a.first[i] - a.first[i0];
    const uint32_t b = done < bq - b0 ? b0 + (uint32_t)done : bq;
    uint32_t err = kNoError;
    span<true>(a, t, e, s.end, s.E, b, bq, &err);
    if (s.first) {
        const uint64_t all = a.first[a.subfirst[s.k + 1]] - a.first[i0];
        if (a.sc.kind == kDCRefine ? all < bq - b0 : all != bq - b0)
            err = err < s.start ? err : s.start;
    }
    return err;
}

// DC first, behind the scan of the differences: the value of unit u, shifted, into the store
__host__ __device__ inline void dcput_lane(const ScanArgs& a, uint32_t u)
{
    uint32_t pos, pos0;
    dd_pos(a.sc, u, pos, pos0);
    a.coef[(size_t)block_of(a.g, a.sc, u) * 64] = (int16_t)((uint32_t)(a.ddoff[pos + 1] - a.ddoff[pos0]) << a.sc.Al);
}

// Behind the last scan the store holds DC VALUES, and the pixel stage of the sequential decoder (k_jdec_dcgather, the scan, k_jdec_idct)
// takes differences along each component with no restart: dcsave copies the values aside, dcdiff writes the differences.
__host__ __device__ inline void dcsave_lane(const ScanArgs& a, uint32_t b)
{
    a.dd[b] = (uint32_t)(int)a.coef[(size_t)b * 64];
}

__host__ __device__ inline void dcdiff_lane(const ScanArgs& a, uint32_t b)
{
    const Geom& g = a.g;
    const uint32_t mcu = b / g.bpm, k = b - mcu * g.bpm;
    uint32_t prev = kNoError;
    if (k < g.ny) {
        const uint32_t pos = mcu * g.ny + k;
        if (pos)
            prev = (pos - 1) / g.ny * g.bpm + (pos - 1) % g.ny;
    } else if (mcu) {
        prev = b - g.bpm;
    }
    a.coef[(size_t)b * 64] = (int16_t)(a.dd[b] - (prev == kNoError ? 0u : a.dd[prev]));
}

}  // namespace jpegprog
}  // namespace v1c
