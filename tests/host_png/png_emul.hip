// png_emul.hip -- TEST HARNESS: runs the product's PNG arithmetic (png_core.hpp: filter, run rule, symbol mapping, token bits) and its
// host-side code builder and planner (png_host.hpp) on the CPU, segment by segment, in the order of the kernels' passes.
//
// Built by tests/test_png_device_host.py itself (hipcc --cuda-host-only -O2 -shared -fPIC, into a temporary directory) and compared there
// with the NumPy restatement of the contract (tests/png_ref.py).  Not part of the product: nothing in vr180_convert_amd/ loads it.
#include <cstring>
#include <vector>

#include "../../include/vr180_remap.h"
#include "../../vr180_convert_amd/csrc/png_host.hpp"

using namespace v1c::png;

namespace {

// one segment as a wave sees it: the bytes and the "equals the byte before" mask
int load_segment(const uint8_t* img, int64_t pitch, const Layout& l, int filter, uint32_t band, uint32_t seg, uint32_t v[kSeg], uint64_t eq[4])
{
    const uint32_t n = l.band_bytes(band), row0 = band * l.band_rows;
    int count = 0;
    eq[0] = eq[1] = eq[2] = eq[3] = 0;
    for (int p = 0; p < kSeg; p++) {
        const uint32_t q = seg * kSeg + p;
        if (q >= n)
            break;
        const uint32_t r = q / l.stride;
        v[p] = filtered_byte(img, pitch, l.bpp, filter, row0 + r, q - r * l.stride);
        if (p && v[p] == v[p - 1])
            eq[p >> 6] |= 1ull << (p & 63);
        count++;
    }
    return count;
}

void or_into(uint8_t* out, uint64_t bitpos, uint64_t value)
{
    value <<= bitpos & 7;
    for (uint64_t b = bitpos >> 3; value; b++, value >>= 8)
        out[b] |= (uint8_t)value;
}

}  // namespace

extern "C" {

void png_emul_code_lengths(const uint64_t* freq, int n, int limit, uint8_t* len)
{
    code_lengths(freq, n, limit, len);
}

uint64_t png_emul_bound(int h, int w, int cn, int depth, int band_rows)
{
    Layout l;
    return make_layout(h, w, cn, depth, band_rows, l) ? bound(l) : 0;
}

// the ABI call's result, computed on the host; `out` holds png_emul_bound bytes.  hist_out: n_bands x 288 counts (may be NULL)
int png_emul_deflate(const uint8_t* img, int h, int w, int64_t pitch, int cn, int depth, int filter, int band_rows, uint8_t* out,
                     v1c_png_band* bands_out, int32_t* n_bands_out, uint64_t* size_out, uint32_t* hist_out)
{
    Layout l;
    if (!make_layout(h, w, cn, depth, band_rows, l))
        return -1;
    std::vector<uint32_t> hist((size_t)l.n_bands * kHistStride, 0);
    std::vector<uint64_t> sums((size_t)l.n_bands * 2, 0);
    uint32_t v[kSeg];
    uint64_t eq[4];
    for (uint32_t b = 0; b < l.n_bands; b++) {
        const uint32_t n = l.band_bytes(b), nseg = (n + kSeg - 1) / kSeg;
        for (uint32_t s = 0; s < nseg; s++) {
            const int cnt = load_segment(img, pitch, l, filter, b, s, v, eq);
            for (int p = 0; p < cnt; p++) {
                int length;
                const int kind = classify(eq, p >> 6, p & 63, &length);
                if (kind != kNone)
                    hist[(size_t)b * kHistStride + token_symbol(kind, v[p], length)]++;
                sums[2 * b] += v[p];
                sums[2 * b + 1] = (sums[2 * b + 1] + (uint64_t)(n - (s * kSeg + p)) * v[p]) % kAdlerBase;
            }
        }
    }
    if (hist_out)
        std::memcpy(hist_out, hist.data(), hist.size() * 4);
    Plan plan;
    plan_image(l, hist.data(), plan);
    std::memset(out, 0, bound(l));
    for (uint32_t b = 0; b < l.n_bands; b++) {
        const uint32_t n = l.band_bytes(b), nseg = (n + kSeg - 1) / kSeg;
        v1c_png_band& r = bands_out[b];
        r.row0 = b * l.band_rows;
        r.row1 = std::min(l.h, r.row0 + l.band_rows);
        r.offset = plan.offset[b];
        r.size = plan.bands[b].size;
        r.adler32 = band_adler(sums[2 * b], sums[2 * b + 1], n);
        r.stored = plan.bands[b].stored;
        uint64_t at = plan.dev[b].token_bit0;  // (the scan: every segment starts where the one before ended)
        for (uint32_t s = 0; s < nseg; s++) {
            const int cnt = load_segment(img, pitch, l, filter, b, s, v, eq);
            for (int p = 0; p < cnt; p++) {
                if (plan.bands[b].stored) {
                    out[plan.dev[b].byte0 + stored_position(s * kSeg + p)] = (uint8_t)v[p];
                    continue;
                }
                int length, nb;
                const int kind = classify(eq, p >> 6, p & 63, &length);
                const uint32_t bits = token_bits(plan.bands[b].table, kind, v[p], length, &nb);
                or_into(out, at, bits);
                at += nb;
            }
        }
    }
    for (const OrWord& o : plan.ors)
        or_into(out, o.word * 32, o.value);
    *n_bands_out = (int32_t)l.n_bands;
    *size_out = plan.total;
    return 0;
}

}
