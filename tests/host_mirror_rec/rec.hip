// Host access to the pair mirror kernel's launch record (csrc/tile_device.hpp: MirrorRec) for tests/test_mirror_record_host.py: the
// product's own __host__ __device__ encode / decode / lane / tap functions, next to the expressions the kernel evaluated per wave
// before the record existed (raw_units_per_row, mirror_raw_fit -- the product's functions too -- and the pass loop of raw_box_dma and
// the fp32 lane mapping of raw_lanes_upr, which are device code and are restated here line by line).
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../vr180_convert_amd/csrc/tile_device.hpp"

using namespace v1c;

static TileBox box_of(const int* v)
{
    TileBox b;
    b.x0 = v[0], b.y0 = v[1], b.cpr = v[2], b.nrows = v[3], b.idx0 = v[4], b.nidx = v[5], b.interior = v[6], b.magic = v[7];
    return b;
}

// raw_box_dma's loop for wave `wave`: the rows its passes start at (first rows of the copies), returns the number of passes
static int passes_of(int R, int nrows, int wave, int* rows_out)
{
    if (nrows > 4096)
        return 0;
    const int rows = R < nrows ? R : nrows;
    const int last0 = nrows - rows;
    int n = 0;
    for (int r0 = wave * R; r0 < nrows; r0 += 4 * R)
        rows_out[n++] = r0 < last0 ? r0 : last0;
    return n;
}

extern "C" {

int rec_sizeof()
{
    return (int)sizeof(MirrorRecWords);
}

void rec_encode(const int* b8, const int* q8, int seq_kb, int one_kb, int src_h, int src_w, uint32_t* out16)
{
    const MirrorRecWords w = mirror_rec_encode(box_of(b8), box_of(q8), seq_kb, one_kb, src_h, src_w);
    std::memcpy(out16, w.w, sizeof(w.w));
}

// out: per box (b at 0, q at 12) y0, x3, nrows, last0, upr, R, nact, magic, lpitch, tapk, passes of waves 0..3 packed (8 bits each),
// the starting rows of wave 0's first two passes packed (16 bits each); then [24] idx0, [25] nidx, [26] flags
void rec_decode(const uint32_t* w16, int64_t* out)
{
    MirrorRecWords w;
    std::memcpy(w.w, w16, sizeof(w.w));
    const MirrorRec r = mirror_rec_decode(w);
    const MirrorRecBox* bx[2] = {&r.b, &r.q};
    for (int k = 0; k < 2; k++) {
        const MirrorRecBox& m = *bx[k];
        int64_t* o = out + 12 * k;
        o[0] = m.y0, o[1] = m.x3, o[2] = m.nrows, o[3] = m.last0, o[4] = m.upr, o[5] = m.R, o[6] = m.nact, o[7] = m.magic, o[8] = m.lpitch,
        o[9] = m.tapk;
        // rec_box_dma's loop
        int64_t packed = 0, rows01 = 0;
        for (int wave = 0; wave < 4; wave++) {
            int n = 0;
            for (int r0 = wave * m.R; r0 < m.nrows; r0 += 4 * m.R) {
                const int rs = r0 < m.last0 ? r0 : m.last0;
                if (wave == 0 && n < 2)
                    rows01 |= (int64_t)rs << (16 * n);
                n++;
            }
            packed |= (int64_t)n << (8 * wave);
        }
        o[10] = packed, o[11] = rows01;
    }
    out[24] = r.idx0, out[25] = r.nidx, out[26] = r.flags;
}

// the same numbers the way the kernel derived them from the TileBox pair (k_ray_lin3_pair_mirror_seq before the record: raw_lanes,
// raw_box_dma, the tap addresses' origin); fit: mirror_raw_fit at `kb`
void rec_present(const int* b8, const int* q8, int kb, int src_h, int src_w, int64_t* out)
{
    const TileBox b = box_of(b8), q = box_of(q8);
    const TileBox* bx[2] = {&b, &q};
    for (int k = 0; k < 2; k++) {
        const TileBox& t = *bx[k];
        int64_t* o = out + 12 * k;
        const int upr = raw_units_per_row(t.cpr);
        if (upr <= 0) {  // (no box: mirror_raw_fit says 0, nothing else is compared)
            for (int i = 0; i < 12; i++)
                o[i] = 0;
            continue;
        }
        const int R = 64 / upr;
        const int rows = R < t.nrows ? R : t.nrows;
        o[0] = t.y0, o[1] = 3 * t.x0, o[2] = t.nrows, o[3] = t.nrows - rows, o[4] = upr, o[5] = R, o[6] = rows * upr, o[7] = 0, o[8] = upr * 16, o[9] = 0;
        int64_t packed = 0, rows01 = 0;
        for (int wave = 0; wave < 4; wave++) {
            static thread_local int rr[4096];  // (boxes far beyond any buffer are asked for their fit verdict too)
            const int n = passes_of(R, t.nrows, wave, rr);
            if (wave == 0)
                for (int i = 0; i < n && i < 2; i++)
                    rows01 |= (int64_t)rr[i] << (16 * i);
            packed |= (int64_t)n << (8 * wave);
        }
        o[10] = packed, o[11] = rows01;
    }
    out[24] = b.idx0, out[25] = b.nidx;
    out[26] = mirror_raw_fit(b, q, kb, src_h, src_w);
}

// exact integer lane -> (row, unit), the record's magic form, and raw_lanes_upr's fp32 form with the reciprocal `ulps` units in the last
// place off the correctly rounded one (v_rcp_f32 is good to one): out[lane] = {row exact, col exact, row magic, row fp32, R fp32}
void rec_lane_forms(int upr, int ulps, int* out)
{
    const uint32_t magic = (65536u + (uint32_t)upr - 1u) / (uint32_t)upr;
    float rupr = 1.0f / (float)upr;
    for (int k = 0; k < (ulps < 0 ? -ulps : ulps); k++)
        rupr = std::nextafterf(rupr, ulps < 0 ? 0.0f : 2.0f);
    for (int lane = 0; lane < 64; lane++) {
        int* o = out + 5 * lane;
        o[0] = lane / upr, o[1] = lane % upr;
        o[2] = (int)mirror_rec_lane_row((uint32_t)lane, magic);
        o[3] = (int)(uint32_t)(((float)lane + 0.5f) * rupr);
        o[4] = (int)(64.5f * rupr);
    }
}

// tap address of a pixel: the record's form on biased coordinate bits against ((sy >> 5) - y0) * pitch + 3 * ((sx >> 5) - x0).
// sx runs over [32 x0, 2^20) with sy fixed at 32 y0 + 7, then sy over [32 y0, 2^20) with sx fixed; returns the number of mismatches
int64_t rec_tap_sweep(int x0, int y0, int cpr)
{
    TileBox t{x0, y0, cpr, 1, 0, 1, 1, 0};
    MirrorRecBox r;
    uint32_t w[5];
    if (!mirror_rec_box(t, r, w))
        return -1;
    const MirrorRecBox d = mirror_rec_unbox(w[0], w[1], w[2], w[3], w[4]);
    const uint32_t pitch = (uint32_t)raw_units_per_row(cpr) * 16u;
    int64_t bad = 0;
    auto one = [&](int sx, int sy) {
        const uint32_t ixb = (uint32_t)((sx >> 5) - x0);
        const uint32_t want = (uint32_t)((sy >> 5) - y0) * pitch + (ixb * 2u + ixb);
        const uint32_t got = mirror_rec_tap((uint32_t)sx + kRoundBias, (uint32_t)sy + kRoundBias, d.lpitch, d.tapk);
        bad += got != want;
    };
    for (int sx = 32 * x0; sx < (1 << 20); sx++)
        one(sx, 32 * y0 + 7);
    for (int sy = 32 * y0; sy < (1 << 20); sy++)
        one(32 * x0 + 13, sy);
    return bad;
}
}
