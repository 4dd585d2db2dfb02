// kernels_mirror.hip -- pairs (apply_lr) and single images of an unrotated chain: one workgroup serves a tile AND the band that
// mirrors it about the equator from one set of coordinates, the boxes brought in by LDS-DMA (k_ray_lin3_pair_mirror_seq: pairs, the
// eyes one after the other through two buffers; k_ray_lin3_pair_mirror_raw: single images; their A/B partners in the tuning build).
// The prologue of the seq and one-eye kernels: the tile from the preloaded head (xcd_tile_at), its row / column loads, then ONE scalar
// load of the tile pair's launch record (MirrorRec, tile_device.hpp) -- fit verdict, table slice, and per box: rows, units per row,
// rows per pass, lanes per pass, the magic of lane -> (row, unit) and the biased origin of the tap addresses -- which plan.hip
// encodes once per plan from the boxes it downloads (tile_mirror_records below).  What is left in the kernel of that arithmetic is
// what belongs to the call: the products with the source and destination pitches.  The A/B partners of the tuning build
// (V1C_MIRROR_REC=0: k_ray_lin3_pair_mirror_seq_box, k_ray_lin3_pair_mirror_box_raw) keep the prologue that decodes the (tile box,
// band box) pair, tests mirror_raw_fit and takes the reciprocals of the units per row in every wave.
// Building blocks: tile_device.hpp.
#include <cmath>

#include "tile_device.hpp"

namespace v1c {

// taps of both eyes of a lane's 4 pixels from the interleaved cells of box `b` (fixed-point rows `sy`), blend, store
// into output row `j`
__device__ __forceinline__ void sample_pair_cells(units_cptr U, const TileIds& t, int j, const TileBox& b, const uint32_t* boxw,
                                                  const int (&sx)[kPX], const int (&sy)[kPX])
{
    typedef uint32_t __attribute__((ext_vector_type(2))) u32x2;
    typedef const __attribute__((address_space(3))) u32x2* lds_u64_ptr;
    const uint32_t lpw8 = (uint32_t)(b.cpr * 4 + 4) * 8u;
    const uint32_t base0 = (uint32_t)(uintptr_t)(lds_u32_ptr)boxw - ((uint32_t)b.y0 * lpw8 + (uint32_t)b.x0 * 8u);
    Taps2 T0, T1;
#pragma unroll
    for (int k = 0; k < kPX; k++) {
        const uint32_t rel = __umul24((uint32_t)(sy[k] >> 5), lpw8) + (((uint32_t)sx[k] >> 2) & ~7u);
        const lds_u64_ptr ra = (lds_u64_ptr)(uintptr_t)(rel + base0), rb = (lds_u64_ptr)(uintptr_t)(rel + base0 + lpw8);
        const u32x2 a_lo = ra[0], a_hi = ra[1], b_lo = rb[0], b_hi = rb[1];
        T0.alo[k] = a_lo.x, T0.ahi[k] = a_hi.x, T0.blo[k] = b_lo.x, T0.bhi[k] = b_hi.x;
        T1.alo[k] = a_lo.y, T1.ahi[k] = a_hi.y, T1.blo[k] = b_lo.y, T1.bhi[k] = b_hi.y;
    }
    uint32_t pix[kPX];
    const uint32_t row_off = (uint32_t)t.x0 * 3u;
#pragma unroll
    for (int e = 0; e < 2; e++) {
#pragma unroll
        for (int k = 0; k < kPX; k++) {
            const BlendW w = blend_weights(sx[k], sy[k]);
            pix[k] = e == 0 ? blend3<4>(T0.alo[k], T0.ahi[k], T0.blo[k], T0.bhi[k], w) : blend3<4>(T1.alo[k], T1.ahi[k], T1.blo[k], T1.bhi[k], w);
        }
        uint8_t* drow = U[e].dst + (__umul24((uint32_t)j, (uint32_t)U[e].dst_pitch) + row_off);
        store4(drow, pix, 0xFu, dst_rows_dword_aligned(U, e));
    }
}

#ifdef V1C_TUNING  // (the register-staged form: A/B partner, V1C_MIRROR_RAW=0, of the LDS-DMA kernels below)
template <int VAR_W>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(5, 8))) void k_ray_lin3_pair_mirror(TileArgs a_)
{
    constexpr int NT = 256;
    __shared__ __attribute__((aligned(16))) double tabw[kTabSlice * kRadialCoefs];
    extern __shared__ __attribute__((aligned(16))) uint32_t dyn_box[];  // one pair of interleaved boxes: 2 x half_dwords
    args_cref a = kernel_args();
    const int tid = threadIdx.x;
    if (blockIdx.z == 0) {  // the tiles the mirror path leaves out, through the general pair code
        const unsigned lin = blockIdx.y * gridDim.x + blockIdx.x;
        if (lin >= (unsigned)a.n_rest)
            return;
        const uint32_t v = ((const V1C_CONST uint32_t*)a.rest_list)[lin];
        shared_map_tile<VAR_W, 0, 2, 0, 1, NT, 0>(a, 2, 2, 0, (int)(v & 0xffffu), (int)(v >> 16), (int)gridDim.x, dyn_box, a.half_dwords,
                                                  tabw, (glb_u32_ptr) nullptr);
        return;
    }
    ctx_cref c = args_ctx(a);
    const units_cptr U = args_units(a);
    const TileBox* __restrict__ boxes = a.boxes;
    const TileBox* __restrict__ mboxes = a.mboxes;
    const int half_dwords = a.half_dwords, mirror_h = a.mirror_h;
    geom_cref g = c.g;
    ray_cref P = c.ray;
    int tx, ty;
    xcd_tile(a.tiles_x_magic, a.strip_len, a.strip_magic, tx, ty);
    ty += 1;  // tile row 0 has no mirror image (row 0 <-> row mirror_h)
    const TileIds t = tile_ids(g, 0, tid, tx, ty, (int)gridDim.x, NT / kLanesX);
    const uint8_t* __restrict__ src0 = U[0].src;
    const uint8_t* __restrict__ src1 = U[1].src;
    const uint32_t pitch0 = (uint32_t)U[0].src_pitch, pitch1 = (uint32_t)U[1].src_pitch;
    const TileBox b = load_tile_box(boxes, t.box_tile), q = load_tile_box(mboxes, t.box_tile);
    if (!mirror_static_ok(b, q, half_dwords, g.src_h, g.src_w))
        return;
    ChunkMap M;
    make_chunk_map<NT>(b, tid, M);
    Staged S0, S1;
    stage_load<false, false>(M, src0, pitch0, 0u, S0);
    stage_load<false, false>(M, src1, pitch1, 0u, S1);
    typedef double __attribute__((ext_vector_type(2))) d2;
    d2 tv = {0.0, 0.0};
    const bool mpoly = (b.interior & 2) != 0;
    if (tid < b.nidx * 4)
        tv = ((const d2*)(radial_table(P, mpoly) + (size_t)b.idx0 * kRadialCoefs))[tid];
    RowCol rc;
    load_rowcol<0>(P, t.xc, t.jc, rc);
    stage_store_pair(M, S0, S1, dyn_box);
    if (tid < b.nidx * 4)
        ((d2*)tabw)[tid] = tv;
    __syncthreads();
    // the mirrored band's box: requested now, in flight while the tile itself is evaluated and sampled
    make_chunk_map<NT>(q, tid, M);
    stage_load<false, false>(M, src0, pitch0, 0u, S0);
    stage_load<false, false>(M, src1, pitch1, 0u, S1);
    LaneCoords L;
    if (mpoly)
        lane_coords<VAR_W, 0, 2, 0, 1, 1, 1>(c, nullptr, rc, kPX, (const double*)tabw, b.idx0, b.nidx, L);
    else
        lane_coords<VAR_W, 0, 2, 0, 1, 0, 1>(c, nullptr, rc, kPX, (const double*)tabw, b.idx0, b.nidx, L);
    sample_pair_cells(U, t, t.j, b, dyn_box, L.sx, L.sy);
    __syncthreads();  // every wave has read its taps of the tile's box
    stage_store_pair(M, S0, S1, dyn_box);
    __syncthreads();
    sample_pair_cells(U, t, mirror_h - t.j, q, dyn_box, L.sx, L.sy2);
}
#endif  // V1C_TUNING

// NE = number of eyes (units) of the launch: 2 = apply_lr's pair; 1 = a single image (apply() of one image, BASELINE config 1):
// the same workgroup with two boxes instead of four
// REC = 1 (the one-eye form): the prologue from the plan's launch record, as in k_ray_lin3_pair_mirror_seq (mirror_seq_tile below)
template <int VAR_W, int NE, int REC>
__device__ __forceinline__ void mirror_raw_tile(V1C_MIRROR_HEAD, double* tabw, uint32_t* dyn_box)
{
    static_assert(!REC || NE == 1, "the record serves the one-eye form");
    constexpr int NT = 256;
    if (V1C_PRIO & 4)
        __builtin_amdgcn_s_setprio(3);
    args_cref a = kernel_args<kMirrorHeadBytes>();
    const int tid = threadIdx.x;
    // grid: first `rest_rows` rows of workgroups for the tiles this path leaves out (general pair code: they take longest, so
    // they are dispatched first -- dispatched last they were a tail: C1 0.0188 -> 0.0245 ms), then the rows of tile pairs
    const unsigned tiles_x = gx_rest & 0xffffu, rest_rows = gx_rest >> 16;
    if (blockIdx.y < rest_rows) {
        const unsigned lin = blockIdx.y * tiles_x + blockIdx.x;
        if (lin >= (unsigned)a.n_rest)
            return;
        const uint32_t v = ((const V1C_CONST uint32_t*)a.rest_list)[lin];
        shared_map_tile<VAR_W, 0, 2, 0, 1, NT, 0>(a, NE, 2, 0, (int)(v & 0xffffu), (int)(v >> 16), (int)tiles_x, dyn_box, a.half_dwords,
                                                  tabw, (glb_u32_ptr) nullptr);
        return;
    }
    // from the preloaded head alone (V1C_MIRROR_HEAD): the tile, its row / column values (vector loads) and its pair of boxes (one scalar
    // load) are requested before the argument block has been read at all
    int tx, ty;
    {
        // strips of 0 / 2 tile rows; floor(2^32 / (2 t)) == floor(floor(2^32 / t) / 2)
        // (REC: the mask tells the compiler what the host knows -- never xcd_tile_at's block mode, whose two divisions then leave the text)
        const unsigned slen = ((rows_strip >> 16) * tiles_x) & (REC ? 0x7fffffffu : 0xffffffffu);
        xcd_tile_at(tiles_x_magic, slen, ((tiles_x_magic - 1u) >> 1) + 1u, tx, ty, rows_strip & 0xffffu, rest_rows, tiles_x, 0u);
    }
    // tile rows 0 .. TY / 2: row 0 of the image has no mirror image (its band row would be row H: not stored), row H / 2 is its
    // own (tile row TY / 2 and its band rewrite rows their neighbours write too -- with the same bytes)
    const DstSize dsz{(int)(dst_wh & 0xffffu), (int)(dst_wh >> 16)};
    const TileIds t = tile_ids(dsz, 0, tid, tx, ty, (int)tiles_x, NT / kLanesX);
    RowCol rc;
    load_rowcol<0>(rowcol_tables_at(rowcol_tables, dsz.dst_w, dsz.dst_h), t.xc, t.jc, rc);
    TileBoxPair bq{};
    MirrorRec r{};
    if constexpr (REC)
        r = load_mirror_rec(pairs, t.box_tile);
    else
        bq = load_tile_box_pair(pairs, t.box_tile);
    const TileBox &b = bq.b, &q = bq.q;
    ctx_cref c = *(const V1C_CONST KernelCtx*)ctxp;
    const units_cptr U = (units_cptr)a.inl;  // (one or two units: always the block's own records, at a known offset)
    geom_cref g = c.g;
    ray_cref P = c.ray;
    touch_plan_and_units<0, NE>(c, U, 0, NE - 1);
    const int nwp = (int)(kb_mh & 0xffffu);
    if (REC ? !(r.flags & kMirrorRecFitOne) : mirror_raw_fit(b, q, nwp, g.src_h, g.src_w) != 1)
        return;
    const bool mpoly = REC ? (r.flags & kMirrorRecMpoly) != 0 : (b.interior & 2) != 0;
    const int idx0 = REC ? r.idx0 : b.idx0, nidx = REC ? r.nidx : b.nidx;
    // (the row / column values are consumed here: the compiler's own wait for them then sits in front of the DMA requests,
    // not -- as vmcnt(0), it does not count LDS-DMA -- in front of the coordinates)
#pragma unroll
    for (int k = 0; k < kPX; k++)
        asm volatile("" ::"v"(rc.slon[k]), "v"(rc.qlon[k]));
    asm volatile("" ::"v"(rc.sl), "v"(rc.cl), "v"(rc.hl));
    const uint32_t lds_tab = (uint32_t)(uintptr_t)(lds_u32_ptr)(const uint32_t*)tabw;
    const uint32_t box_bytes = (uint32_t)nwp * 1024u;
    // (one image: two boxes -- half the LDS of a pair's workgroup, 7 workgroups per CU at 67 VGPRs)
    const uint32_t raw_b = (uint32_t)(uintptr_t)(lds_u32_ptr)dyn_box, raw_q = raw_b + (uint32_t)NE * box_bytes;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    {  // table slice: nidx * 4 units of 16 bytes, one pass (units past the slice: clamped, they land in the unused tail of tabw)
        const uint32_t u = min((uint32_t)tid, (uint32_t)(nidx * 4 - 1));
        const uint8_t* gp = (const uint8_t*)(radial_table(P, mpoly) + (size_t)idx0 * kRadialCoefs) + u * 16u;
        __builtin_amdgcn_global_load_lds((glb_void_ptr)gp, (lds_void_ptr)(uintptr_t)(lds_tab + (uint32_t)__builtin_amdgcn_readfirstlane(tid & ~63) * 16u), 16, 0, 0);
    }
    const RawLanes mb = REC ? rec_lanes(r.b, lane) : raw_lanes(b.cpr, lane), mq = REC ? rec_lanes(r.q, lane) : raw_lanes(q.cpr, lane);
    const uint32_t row_off = (uint32_t)t.x0 * 3u;
    const int mirror_h = (int)(kb_mh >> 16);
    const int jm = mirror_h - t.j;              // the band's row
    const bool band_row = jm < dsz.dst_h;         // (false for row 0 of the image only)
    LaneCoords L;
    uint32_t p0[kPX], p1[kPX];
    int nb, nq;
    if constexpr (REC) {
        nb = rec_box_dma(r.b, mb, U[0].src, (uint32_t)U[0].src_pitch, lane, wave, raw_b);
        nq = rec_box_dma(r.q, mq, U[0].src, (uint32_t)U[0].src_pitch, lane, wave, raw_q);
    } else {
        nb = raw_box_dma(b, mb, U[0].src, (uint32_t)U[0].src_pitch, lane, wave, raw_b);  // this wave's requests per box of the tile ...
        if (NE == 2)
            raw_box_dma(b, mb, U[NE - 1].src, (uint32_t)U[NE - 1].src_pitch, lane, wave, raw_b + box_bytes);
        nq = raw_box_dma(q, mq, U[0].src, (uint32_t)U[0].src_pitch, lane, wave, raw_q);  // ... and of the mirrored band
        if (NE == 2)
            raw_box_dma(q, mq, U[NE - 1].src, (uint32_t)U[NE - 1].src_pitch, lane, wave, raw_q + box_bytes);
    }
    if (V1C_PRIO & 4)
        __builtin_amdgcn_s_setprio(0);
    // Barriers without __syncthreads()' fence (it would wait for every load in flight): each wave waits for its own part of
    // what the barrier publishes -- vmcnt counts in issue order -- then joins.
    wait_vm_barrier(NE * (nb + nq));  // table slice landed (this wave's box loads may still be in flight)
    if (mpoly)
        lane_coords<VAR_W, 0, 2, 0, 1, 1, 1, 0, REC>(c, nullptr, rc, kPX, (const double*)tabw, idx0, nidx, L);
    else
        lane_coords<VAR_W, 0, 2, 0, 1, 0, 1, 0, REC>(c, nullptr, rc, kPX, (const double*)tabw, idx0, nidx, L);
    wait_vm_barrier(NE * nq);  // the tile's boxes
    if constexpr (NE == 2) {
        gather_pair_raw(b, raw_b, box_bytes, L.sx, L.sy, p0, p1);
        // the mirrored band's boxes: waited for BEFORE the tile's stores are issued (stores count in vmcnt too)
        wait_vm_barrier_imm<0>();
        store_pair_row(U, t, t.j, p0, p1);
        gather_pair_raw(q, raw_q, box_bytes, L.sx, L.sy2, p0, p1);
        if (band_row)
            store_pair_row(U, t, jm, p0, p1);
    } else if constexpr (REC) {
        gather_one_rec(r.b, raw_b, L.sx, L.sy, p0);
        wait_vm_barrier_imm<0>();
        store4<1>(U[0].dst + (mul24_vs((uint32_t)t.j, (uint32_t)U[0].dst_pitch) + row_off), p0, 0xFu, dst_rows_dword_aligned(U, 0));
        gather_one_rec(r.q, raw_q, L.sx, L.sy2, p1);
        if (band_row)
            store4<1>(U[0].dst + (mul24_vs((uint32_t)jm, (uint32_t)U[0].dst_pitch) + row_off), p1, 0xFu, dst_rows_dword_aligned(U, 0));
    } else {
        gather_one_raw(b, raw_b, L.sx, L.sy, p0);
        wait_vm_barrier_imm<0>();
        store4<1>(U[0].dst + (__umul24((uint32_t)t.j, (uint32_t)U[0].dst_pitch) + row_off), p0, 0xFu, dst_rows_dword_aligned(U, 0));
        gather_one_raw(q, raw_q, L.sx, L.sy2, p1);
        if (band_row)
            store4<1>(U[0].dst + (__umul24((uint32_t)jm, (uint32_t)U[0].dst_pitch) + row_off), p1, 0xFu, dst_rows_dword_aligned(U, 0));
    }
}

template <int VAR_W, int NE = 2>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(V1C_RAW_WAVES, 8))) void k_ray_lin3_pair_mirror_raw(V1C_MIRROR_HEAD, TileArgs a_)
{
    __shared__ __attribute__((aligned(16))) double tabw[kTabSlice * kRadialCoefs];
    extern __shared__ __attribute__((aligned(16))) uint32_t dyn_box[];  // 2 NE raw boxes (or the general code's cell buffers)
    mirror_raw_tile<VAR_W, NE, NE == 1>(pairs, tiles_x_magic, gx_rest, rows_strip, dst_wh, rowcol_tables, ctxp, kb_mh, tabw, dyn_box);
}
#ifdef V1C_TUNING  // (V1C_MIRROR_REC=0: the one-eye form on the plain box pairs)
template <int VAR_W>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(V1C_RAW_WAVES, 8))) void k_ray_lin3_pair_mirror_box_raw(V1C_MIRROR_HEAD, TileArgs a_)
{
    __shared__ __attribute__((aligned(16))) double tabw[kTabSlice * kRadialCoefs];
    extern __shared__ __attribute__((aligned(16))) uint32_t dyn_box[];
    mirror_raw_tile<VAR_W, 1, 0>(pairs, tiles_x_magic, gx_rest, rows_strip, dst_wh, rowcol_tables, ctxp, kb_mh, tabw, dyn_box);
}
#endif

// ---- the pair kernel with the eyes one after the other: two box buffers instead of four ----
// k_ray_lin3_pair_mirror_raw holds four boxes (two eyes x tile and band) in LDS at once.  Here the workgroup keeps two buffers (tile
// box, band box) and serves eye 0, then eye 1 with the SAME tap addresses and weights (one map per call: both eyes read the same
// box positions), requesting eye 1's tile box as soon as every wave has sampled eye 0's, and its band box likewise:
//   requests: table slice, b(eye 0), q(eye 0) | coordinates -> tap addresses + weights of tile and band (24 registers)
//   gather b | -> request b(eye 1) | store | gather q | -> request q(eye 1) | store | gather b | store | gather q | store
// With the LDS of the four-box form each buffer holds boxes of twice the size -- the pairs that went to the general pair code for
// their size (2 % of the tiles, 3 - 6 % of a C2 launch) stay here -- or, with the same capacity, a workgroup takes half the LDS
// (C1's 9 KB boxes: 4 -> 6 workgroups per CU); a gather holds one eye's taps (24 registers instead of 48).
#ifndef V1C_SEQ_WAVES
#define V1C_SEQ_WAVES 6
#endif
__device__ __forceinline__ void gather_taps_raw(const uint32_t (&ta)[kPX], const BlendW (&W)[kPX], uint32_t pitch, uint32_t (&pix)[kPX])
{
#pragma unroll
    for (int k = 0; k < kPX; k++) {
        const uint32_t a = ta[k], d = a & ~3u;
        const lds_u32_ptr r0 = (lds_u32_ptr)(uintptr_t)d, r1 = (lds_u32_ptr)(uintptr_t)(d + pitch);
        const uint32_t a0 = r0[0], a1 = r0[1], a2 = r0[2], b0 = r1[0], b1 = r1[1], b2 = r1[2];
        pix[k] = blend3<3>(__builtin_amdgcn_alignbyte(a1, a0, a), __builtin_amdgcn_alignbyte(a2, a1, a), __builtin_amdgcn_alignbyte(b1, b0, a),
                           __builtin_amdgcn_alignbyte(b2, b1, a), W[k]);
    }
}

// REC = 1: the prologue from the plan's launch record (MirrorRec, tile_device.hpp): fit verdict, units per row, rows per pass, the
// lanes' (row, unit) of a pass by a 16-bit magic and the biased box origins of the tap addresses come out of the record's one scalar
// load; the coordinates stay the rounding trick's raw bits (lane_coords<..., BIASED>), a tap address is one shift and one 24-bit
// multiply-add per box on top of the 3 (bx >> 5) both boxes share, and the destination row offsets are 24-bit multiplies too.
// REC = 0 (tuning build, V1C_MIRROR_REC=0): the prologue that decodes the (tile box, band box) pair in every wave -- the A/B partner.
// Requests, stores and waits are the same in both: row / column loads, table slice, b, q | ... (see above).
template <int VAR_W, int REST, int REC>
__device__ __forceinline__ void mirror_seq_tile(V1C_MIRROR_HEAD, double* tabw, uint32_t* dyn_box)
{
    constexpr int NT = 256;
    if (V1C_PRIO & 4)
        __builtin_amdgcn_s_setprio(3);
    args_cref a = kernel_args<kMirrorHeadBytes>();
    const int tid = threadIdx.x;
    const unsigned tiles_x = gx_rest & 0xffffu, rest_rows = REST ? gx_rest >> 16 : 0u;
    if constexpr (REST) {
        if (blockIdx.y < rest_rows) {
            const unsigned lin = blockIdx.y * tiles_x + blockIdx.x;
            if (lin >= (unsigned)a.n_rest)
                return;
            const uint32_t v = ((const V1C_CONST uint32_t*)a.rest_list)[lin];
            shared_map_tile<VAR_W, 0, 2, 0, 1, NT, 0>(a, 2, 2, 0, (int)(v & 0xffffu), (int)(v >> 16), (int)tiles_x, dyn_box,
                                                      a.half_dwords, tabw, (glb_u32_ptr) nullptr);
            return;
        }
    }
    // from the preloaded head alone (V1C_MIRROR_HEAD): the tile, its row / column values (vector loads) and its record (one scalar
    // load) are requested before the argument block has been read at all
    int tx, ty;
    {
        // strips of 0 / 2 tile rows; floor(2^32 / (2 t)) == floor(floor(2^32 / t) / 2)
        // (REC: the mask tells the compiler what the host knows -- never xcd_tile_at's block mode, whose two divisions then leave the text)
        const unsigned slen = ((rows_strip >> 16) * tiles_x) & (REC ? 0x7fffffffu : 0xffffffffu);
        xcd_tile_at(tiles_x_magic, slen, ((tiles_x_magic - 1u) >> 1) + 1u, tx, ty, rows_strip & 0xffffu, rest_rows, tiles_x, 0u);
    }
    // tile rows 0 .. TY / 2: row 0 of the image has no mirror image (its band row would be row H: not stored), row H / 2 is its
    // own (tile row TY / 2 and its band rewrite rows their neighbours write too -- with the same bytes)
    const DstSize dsz{(int)(dst_wh & 0xffffu), (int)(dst_wh >> 16)};
    const TileIds t = tile_ids(dsz, 0, tid, tx, ty, (int)tiles_x, NT / kLanesX);
    RowCol rc;
    load_rowcol<0>(rowcol_tables_at(rowcol_tables, dsz.dst_w, dsz.dst_h), t.xc, t.jc, rc);
    TileBoxPair bq{};
    MirrorRec r{};
    if constexpr (REC)
        r = load_mirror_rec(pairs, t.box_tile);
    else
        bq = load_tile_box_pair(pairs, t.box_tile);
    const TileBox &b = bq.b, &q = bq.q;
    ctx_cref c = *(const V1C_CONST KernelCtx*)ctxp;
    const units_cptr U = (units_cptr)a.inl;  // (one or two units: always the block's own records, at a known offset)
    geom_cref g = c.g;
    ray_cref P = c.ray;
    touch_plan_and_units<0, 2>(c, U, 0, 1);
    const int cap_kb = (int)(kb_mh & 0xffffu);
    if (REC ? !(r.flags & kMirrorRecFitSeq) : mirror_raw_fit(b, q, cap_kb, g.src_h, g.src_w) != 1)
        return;
    const bool mpoly = REC ? (r.flags & kMirrorRecMpoly) != 0 : (b.interior & 2) != 0;
    const int idx0 = REC ? r.idx0 : b.idx0, nidx = REC ? r.nidx : b.nidx;
#pragma unroll
    for (int k = 0; k < kPX; k++)
        asm volatile("" ::"v"(rc.slon[k]), "v"(rc.qlon[k]));
    asm volatile("" ::"v"(rc.sl), "v"(rc.cl), "v"(rc.hl));
    const uint32_t lds_tab = (uint32_t)(uintptr_t)(lds_u32_ptr)(const uint32_t*)tabw;
    const uint32_t raw_b = (uint32_t)(uintptr_t)(lds_u32_ptr)dyn_box, raw_q = raw_b + (uint32_t)cap_kb * 1024u;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    {
        const uint32_t u = min((uint32_t)tid, (uint32_t)(nidx * 4 - 1));
        const uint8_t* gp = (const uint8_t*)(radial_table(P, mpoly) + (size_t)idx0 * kRadialCoefs) + u * 16u;
        __builtin_amdgcn_global_load_lds((glb_void_ptr)gp, (lds_void_ptr)(uintptr_t)(lds_tab + (uint32_t)__builtin_amdgcn_readfirstlane(tid & ~63) * 16u), 16, 0, 0);
    }
    const RawLanes mb = REC ? rec_lanes(r.b, lane) : raw_lanes(b.cpr, lane), mq = REC ? rec_lanes(r.q, lane) : raw_lanes(q.cpr, lane);
    // one eye's (tile box, band box) requests; returns the band's count (the tile's in `nb`)
    auto request = [&](int e, int which) {
        const uint8_t* src = U[e].src;
        const uint32_t sp = (uint32_t)U[e].src_pitch;
        if constexpr (REC)
            return which == 0 ? rec_box_dma(r.b, mb, src, sp, lane, wave, raw_b) : rec_box_dma(r.q, mq, src, sp, lane, wave, raw_q);
        else
            return which == 0 ? raw_box_dma(b, mb, src, sp, lane, wave, raw_b) : raw_box_dma(q, mq, src, sp, lane, wave, raw_q);
    };
    const int nb = request(0, 0);
    const int nq = request(0, 1);
    if (V1C_PRIO & 4)
        __builtin_amdgcn_s_setprio(0);
    wait_vm_barrier(nb + nq);  // table slice
    const uint32_t pitch_b = REC ? r.b.lpitch : (uint32_t)raw_units_per_row(b.cpr) * 16u, pitch_q = REC ? r.q.lpitch : (uint32_t)raw_units_per_row(q.cpr) * 16u;
    uint32_t ta_b[kPX], ta_q[kPX];
    BlendW W_b[kPX], W_q[kPX];
    {
        LaneCoords L;
        if (mpoly)
            lane_coords<VAR_W, 0, 2, 0, 1, 1, 1, 0, REC>(c, nullptr, rc, kPX, (const double*)tabw, idx0, nidx, L);
        else
            lane_coords<VAR_W, 0, 2, 0, 1, 0, 1, 0, REC>(c, nullptr, rc, kPX, (const double*)tabw, idx0, nidx, L);
        const uint32_t kb = r.b.tapk + raw_b, kq = r.q.tapk + raw_q;  // (REC)
#pragma unroll
        for (int k = 0; k < kPX; k++) {
            if constexpr (REC) {  // (mirror_rec_tap: the coordinates carry the rounding bias, the origins its image)
                const uint32_t bx = ((uint32_t)L.sx[k] >> 5), x3 = bx * 2u + bx;
                ta_b[k] = mad24_vsv((uint32_t)L.sy[k] >> 5, pitch_b, x3 + kb);
                ta_q[k] = mad24_vsv((uint32_t)L.sy2[k] >> 5, pitch_q, x3 + kq);
            } else {
                const uint32_t ixb = (uint32_t)((L.sx[k] >> 5) - b.x0), ixq = (uint32_t)((L.sx[k] >> 5) - q.x0);
                ta_b[k] = __umul24((uint32_t)((L.sy[k] >> 5) - b.y0), pitch_b) + (ixb * 2u + ixb) + raw_b;
                ta_q[k] = __umul24((uint32_t)((L.sy2[k] >> 5) - q.y0), pitch_q) + (ixq * 2u + ixq) + raw_q;
            }
            W_b[k] = blend_weights(L.sx[k], L.sy[k]);
            W_q[k] = blend_weights(L.sx[k], L.sy2[k]);
        }
    }
    const uint32_t row_off = (uint32_t)t.x0 * 3u;
    const int jm = (int)(kb_mh >> 16) - t.j;
    const bool band_row = jm < dsz.dst_h;
    // byte offset of row j of eye e's destination (j and the pitch are below 2^24)
    auto drow = [&](int e, int j) {
        return (REC ? mul24_vs((uint32_t)j, (uint32_t)U[e].dst_pitch) : __umul24((uint32_t)j, (uint32_t)U[e].dst_pitch)) + row_off;
    };
    uint32_t pix[kPX];
    // ---- eye 0 ----
    wait_vm_barrier(nq);  // tile box
    gather_taps_raw(ta_b, W_b, pitch_b, pix);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");  // band box landed; every wave has sampled the tile box
    request(1, 0);
    store4<1>(U[0].dst + drow(0, t.j), pix, 0xFu, dst_rows_dword_aligned(U, 0));
    gather_taps_raw(ta_q, W_q, pitch_q, pix);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // every wave has sampled the band box
    request(1, 1);
    if (band_row)
        store4<1>(U[0].dst + drow(0, jm), pix, 0xFu, dst_rows_dword_aligned(U, 0));
    // ---- eye 1 (behind its tile box: eye 0's tile store and its band's nq requests; the predicated band store is not counted) ----
    wait_vm_barrier(nq + 1);
    gather_taps_raw(ta_b, W_b, pitch_b, pix);
    wait_vm_barrier_imm<0>();
    store4<1>(U[1].dst + drow(1, t.j), pix, 0xFu, dst_rows_dword_aligned(U, 1));
    gather_taps_raw(ta_q, W_q, pitch_q, pix);
    if (band_row)
        store4<1>(U[1].dst + drow(1, jm), pix, 0xFu, dst_rows_dword_aligned(U, 1));
}

// REST = 0: the plan's rest list is empty (C2: every tile pair fits) -- the instantiation without the general pair code, whose
// registers (74 against 68 VGPRs, 94 against 66 SGPRs) and LDS (its cell buffers) otherwise set the occupancy of a launch that never
// runs it: 7 instead of 6 workgroups per CU
template <int VAR_W, int REST = 1>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(REST ? V1C_SEQ_WAVES : V1C_SEQ_WAVES + 1, 8))) void k_ray_lin3_pair_mirror_seq(V1C_MIRROR_HEAD, TileArgs a_)
{
    __shared__ __attribute__((aligned(16))) double tabw[kTabSlice * kRadialCoefs];
    extern __shared__ __attribute__((aligned(16))) uint32_t dyn_box[];  // 2 raw boxes of a.kb KB (or the general code's cell buffers)
    mirror_seq_tile<VAR_W, REST, 1>(pairs, tiles_x_magic, gx_rest, rows_strip, dst_wh, rowcol_tables, ctxp, kb_mh, tabw, dyn_box);
}
#ifdef V1C_TUNING  // (V1C_MIRROR_REC=0: `pairs` = the plain box pairs)
template <int VAR_W, int REST = 1>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(REST ? V1C_SEQ_WAVES : V1C_SEQ_WAVES + 1, 8))) void k_ray_lin3_pair_mirror_seq_box(V1C_MIRROR_HEAD, TileArgs a_)
{
    __shared__ __attribute__((aligned(16))) double tabw[kTabSlice * kRadialCoefs];
    extern __shared__ __attribute__((aligned(16))) uint32_t dyn_box[];
    mirror_seq_tile<VAR_W, REST, 0>(pairs, tiles_x_magic, gx_rest, rows_strip, dst_wh, rowcol_tables, ctxp, kb_mh, tabw, dyn_box);
}
#endif

// ---- the seq kernel on a plan's tap table (tap_table.hpp) ----
// The lane's map evaluation -- row / column loads, the radial-table slice and its barrier phase, the fp64 coordinates -- depends on the
// plan only; for plans without rest tiles plan.hip has it done once (k_fill_tap_table below) and keeps 12 bytes per lane.  This kernel is
// mirror_seq_tile<., REST = 0, REC = 1> with that block replaced: the wave's first request brings its own 64 entries (768 bytes) into a
// 3 KB area that takes the place of the table slice, the first counted wait publishes them as it published the slice, and each lane
// decodes its entry into the same 8 tap addresses and 8 weight pairs.  One instantiation: VAR_W and the polynomial's variable are the
// fill's business.  Requests, stores and waits behind the decode are the computing kernel's, statement by statement.
// (The 768 bytes travel as 48 lanes of the 16-byte form: lane-linear in LDS, which the 12-byte form is not -- tools/ubench/dma_raw_forms.hip.)
// EB = 8, the compact entry (TapEntry8): the same body; lanes 0 .. 31 of a wave issue the request (512 bytes), a lane reads its entry
// with one 8-byte LDS read, the area is 2 KB, and the decode takes the tile pair's K from the record that came with the first scalar load.
constexpr int kTapSliceBytes = 256 * kTapEntryBytes, kTap8SliceBytes = 256 * kTap8EntryBytes;
template <int EB>
__device__ __forceinline__ void mirror_seq_tab_tile(V1C_MIRROR_HEAD, uint32_t* tapw, uint32_t* dyn_box)
{
    static_assert(EB == kTapEntryBytes || EB == kTap8EntryBytes, "the 12-byte entry or the compact one");
    constexpr int NT = 256;
    if (V1C_PRIO & 4)
        __builtin_amdgcn_s_setprio(3);
    args_cref a = kernel_args<kMirrorHeadBytes>();
    const int tid = threadIdx.x;
    const unsigned tiles_x = gx_rest & 0xffffu;
    int tx, ty;
    {
        const unsigned slen = ((rows_strip >> 16) * tiles_x) & 0x7fffffffu;
        xcd_tile_at(tiles_x_magic, slen, ((tiles_x_magic - 1u) >> 1) + 1u, tx, ty, rows_strip & 0xffffu, 0u, tiles_x, 0u);
    }
    const DstSize dsz{(int)(dst_wh & 0xffffu), (int)(dst_wh >> 16)};
    const TileIds t = tile_ids(dsz, 0, tid, tx, ty, (int)tiles_x, NT / kLanesX);
    const MirrorRec r = load_mirror_rec(pairs, t.box_tile);
    const units_cptr U = (units_cptr)a.inl;
    // the pair's pointers and pitches, read in one clause next to the record and held as values: left as loads, the compiler reads eye 1's
    // source and both destinations again behind the barriers, where each is a round trip in front of a request or a store
    const uint8_t* usrc[2] = {U[0].src, U[1].src};
    uint8_t* udst[2] = {U[0].dst, U[1].dst};
    uint32_t uspitch[2] = {(uint32_t)U[0].src_pitch, (uint32_t)U[1].src_pitch}, udpitch[2] = {(uint32_t)U[0].dst_pitch, (uint32_t)U[1].dst_pitch};
    asm volatile("" : "+s"(usrc[0]), "+s"(usrc[1]), "+s"(udst[0]), "+s"(udst[1]), "+s"(uspitch[0]), "+s"(uspitch[1]), "+s"(udpitch[0]), "+s"(udpitch[1]));
    const bool ualigned[2] = {((((uintptr_t)udst[0]) | (uintptr_t)udpitch[0]) & 3u) == 0, ((((uintptr_t)udst[1]) | (uintptr_t)udpitch[1]) & 3u) == 0};
    const int cap_kb = (int)(kb_mh & 0xffffu);
    if (!(r.flags & kMirrorRecFitSeq))
        return;
    const uint32_t lds_tap = (uint32_t)(uintptr_t)(lds_u32_ptr)(const uint32_t*)tapw;
    const uint32_t raw_b = (uint32_t)(uintptr_t)(lds_u32_ptr)dyn_box, raw_q = raw_b + (uint32_t)cap_kb * 1024u;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    {  // this wave's 64 entries: the table is lane-linear within a tile pair (`rowcol_tables` of the head carries its base)
        const uint32_t wave_off = (uint32_t)__builtin_amdgcn_readfirstlane(tid & ~63) * (uint32_t)EB;
        const uint8_t* gp = (const uint8_t*)rowcol_tables + ((size_t)(uint32_t)__builtin_amdgcn_readfirstlane(t.box_tile) * (size_t)(256 * EB) + wave_off) +
                            (uint32_t)lane * 16u;
        if (lane < 64 * EB / 16)
            __builtin_amdgcn_global_load_lds((glb_void_ptr)gp, (lds_void_ptr)(uintptr_t)(lds_tap + wave_off), 16, 0, 0);
    }
    const RawLanes mb = rec_lanes(r.b, lane), mq = rec_lanes(r.q, lane);
    auto request = [&](int e, int which) {
        const uint8_t* src = usrc[e];
        const uint32_t sp = uspitch[e];
        return which == 0 ? rec_box_dma(r.b, mb, src, sp, lane, wave, raw_b) : rec_box_dma(r.q, mq, src, sp, lane, wave, raw_q);
    };
    const int nb = request(0, 0);
    const int nq = request(0, 1);
    if (V1C_PRIO & 4)
        __builtin_amdgcn_s_setprio(0);
    wait_vm_barrier(nb + nq);  // the entries
    const uint32_t pitch_b = r.b.lpitch, pitch_q = r.q.lpitch;
    uint32_t ta_b[kPX], ta_q[kPX];
    BlendW W_b[kPX], W_q[kPX];
    {
        TapCoords tc;
        if constexpr (EB == kTap8EntryBytes) {
            typedef uint32_t __attribute__((ext_vector_type(2))) u32x2;
            typedef const __attribute__((address_space(3))) u32x2* lds_u64_ptr;
            const u32x2 ev = *(lds_u64_ptr)(uintptr_t)(lds_tap + (uint32_t)tid * (uint32_t)EB);
            tc = tap8_decode(TapEntry8{{ev.x, ev.y}}, r.tap_k);
        } else {
            const lds_u32_ptr ep = (lds_u32_ptr)(uintptr_t)(lds_tap + (uint32_t)tid * (uint32_t)EB);
            tc = tap_entry_decode(TapEntry{{ep[0], ep[1], ep[2]}});
        }
        const uint32_t kb = raw_b, kq = raw_q + (uint32_t)(r.b.x3 - r.q.x3);
#pragma unroll
        for (int k = 0; k < kPX; k++) {
            const uint32_t ix = (uint32_t)tc.x[k] >> 5, x3 = ix * 2u + ix;
            ta_b[k] = mad24_vsv((uint32_t)tc.y[k] >> 5, pitch_b, x3 + kb);
            ta_q[k] = mad24_vsv((uint32_t)tc.y2[k] >> 5, pitch_q, x3 + kq);
            W_b[k] = blend_weights(tc.x[k], tc.y[k]);
            W_q[k] = blend_weights(tc.x[k], tc.y2[k]);
        }
    }
    const uint32_t row_off = (uint32_t)t.x0 * 3u;
    const int jm = (int)(kb_mh >> 16) - t.j;
    const bool band_row = jm < dsz.dst_h;
    auto drow = [&](int e, int j) { return mul24_vs((uint32_t)j, udpitch[e]) + row_off; };
    uint32_t pix[kPX];
    // ---- eye 0 ----
    wait_vm_barrier(nq);  // tile box
    gather_taps_raw(ta_b, W_b, pitch_b, pix);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");  // band box landed; every wave has sampled the tile box
    request(1, 0);
    store4<1>(udst[0] + drow(0, t.j), pix, 0xFu, ualigned[0]);
    gather_taps_raw(ta_q, W_q, pitch_q, pix);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");  // every wave has sampled the band box
    request(1, 1);
    if (band_row)
        store4<1>(udst[0] + drow(0, jm), pix, 0xFu, ualigned[0]);
    // ---- eye 1 (behind its tile box: eye 0's tile store and its band's nq requests; the predicated band store is not counted) ----
    wait_vm_barrier(nq + 1);
    gather_taps_raw(ta_b, W_b, pitch_b, pix);
    wait_vm_barrier_imm<0>();
    store4<1>(udst[1] + drow(1, t.j), pix, 0xFu, ualigned[1]);
    gather_taps_raw(ta_q, W_q, pitch_q, pix);
    if (band_row)
        store4<1>(udst[1] + drow(1, jm), pix, 0xFu, ualigned[1]);
}

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(V1C_SEQ_WAVES + 1, 8))) void k_ray_lin3_pair_mirror_seq_tab(V1C_MIRROR_HEAD, TileArgs a_)
{
    __shared__ __attribute__((aligned(16))) uint32_t tapw[kTapSliceBytes / 4];
    extern __shared__ __attribute__((aligned(16))) uint32_t dyn_box[];  // 2 raw boxes of a.kb KB
    mirror_seq_tab_tile<kTapEntryBytes>(pairs, tiles_x_magic, gx_rest, rows_strip, dst_wh, rowcol_tables, ctxp, kb_mh, tapw, dyn_box);
}
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(V1C_SEQ_WAVES + 1, 8))) void k_ray_lin3_pair_mirror_seq_tab8(V1C_MIRROR_HEAD, TileArgs a_)
{
    __shared__ __attribute__((aligned(16))) uint32_t tapw[kTap8SliceBytes / 4];
    extern __shared__ __attribute__((aligned(16))) uint32_t dyn_box[];
    mirror_seq_tab_tile<kTap8EntryBytes>(pairs, tiles_x_magic, gx_rest, rows_strip, dst_wh, rowcol_tables, ctxp, kb_mh, tapw, dyn_box);
}

// The fill: one workgroup per tile pair of tile rows 0 .. TY / 2, the lanes laid out as the mirror kernels lay them out (tile_ids), the
// coordinates by the instantiation of lane_coords the seq kernel runs for this plan and tile (VAR_W; the tile's polynomial variable; the
// tile's table slice, read where it lies), rebased on the box origins and packed.  A lane whose values do not fit an entry raises
// `*overflow`: the plan then drops the table.  `entry_bytes`: 12, or 8 -- the compact entry, whose K is the record's (`tap_s`: the plan's S).
template <int VAR_W>
__global__ __launch_bounds__(256) void k_fill_tap_table(const KernelCtx* ctxp, const TileBox* __restrict__ boxes, const TileBox* __restrict__ mboxes,
                                                        int tiles_x, uint32_t* __restrict__ table, uint32_t* overflow, int entry_bytes, int tap_s)
{
    ctx_cref c = *(const V1C_CONST KernelCtx*)ctxp;
    ray_cref P = c.ray;
    const int tid = threadIdx.x;
    const TileIds t = tile_ids(c.g, 0, tid, (int)blockIdx.x, (int)blockIdx.y, tiles_x, 256 / kLanesX);
    const TileBox b = boxes[t.box_tile], q = mboxes[t.box_tile];
    RowCol rc;
    load_rowcol<0>(P, t.xc, t.jc, rc);
    const bool mpoly = (b.interior & 2) != 0;
    const int nidx = max(b.nidx, 1), idx0 = max(b.idx0, 0);
    const double* tab = (mpoly ? P.radial_m : P.radial) + (size_t)idx0 * kRadialCoefs;
    LaneCoords L;
    if (mpoly)
        lane_coords<VAR_W, 0, 2, 0, 1, 1, 1, 0, 1>(c, nullptr, rc, kPX, tab, idx0, nidx, L);
    else
        lane_coords<VAR_W, 0, 2, 0, 1, 0, 1, 0, 1>(c, nullptr, rc, kPX, tab, idx0, nidx, L);
    TapCoords tc;
#pragma unroll
    for (int k = 0; k < kPX; k++) {
        tc.x[k] = (int)((uint32_t)L.sx[k] - kRoundBias) - 32 * b.x0;
        tc.y[k] = (int)((uint32_t)L.sy[k] - kRoundBias) - 32 * b.y0;
        tc.y2[k] = (int)((uint32_t)L.sy2[k] - kRoundBias) - 32 * q.y0;
    }
    const size_t at = (size_t)t.box_tile * 256u + (size_t)tid;
    if (entry_bytes == kTap8EntryBytes) {
        const int K = tap_s - 32 * (b.y0 + q.y0);  // (mirror_rec_encode's expression)
        if (!tap8_fits(tc, K))
            atomicOr(overflow, 1u);
        const TapEntry8 e = tap8_encode(tc, K);
        uint32_t* out = table + at * 2u;
        out[0] = e.w[0], out[1] = e.w[1];
        return;
    }
    if (!tap_entry_fits(tc))
        atomicOr(overflow, 1u);
    const TapEntry e = tap_entry_encode(tc);
    uint32_t* out = table + at * 3u;
    out[0] = e.w[0], out[1] = e.w[1], out[2] = e.w[2];
}

size_t tap_table_bytes(const Geom& g, int entry_bytes)
{
    const dim3 full = tile_grid(g, 256, 1);
    return (size_t)full.x * (size_t)(full.y / 2 + 1) * 256u * (size_t)entry_bytes;
}

int tap_table_s(const KernelCtx& c)
{
    const double s = 2.0 * c.ray.cy32;  // 64 x the row centre
    return std::fabs(s) < 1.0e9 ? (int)std::llrint(s) : 0;
}

hipError_t launch_fill_tap_table(const KernelCtx& c, const KernelCtx* cdev, const void* boxes, const void* mboxes, void* table, uint32_t* overflow,
                                 int entry_bytes)
{
    if (entry_bytes != kTapEntryBytes && entry_bytes != kTap8EntryBytes)
        return hipErrorInvalidValue;
    const dim3 full = tile_grid(c.g, 256, 1);
    const dim3 grid(full.x, full.y / 2 + 1, 1), block(256, 1, 1);
    const int tap_s = tap_table_s(c);
    if (c.ray.var_is_w)
        hipLaunchKernelGGL((k_fill_tap_table<1>), grid, block, 0, 0, cdev, (const TileBox*)boxes, (const TileBox*)mboxes, (int)full.x, (uint32_t*)table, overflow,
                           entry_bytes, tap_s);
    else
        hipLaunchKernelGGL((k_fill_tap_table<0>), grid, block, 0, 0, cdev, (const TileBox*)boxes, (const TileBox*)mboxes, (int)full.x, (uint32_t*)table, overflow,
                           entry_bytes, tap_s);
    return hipGetLastError();
}

// Rest list of the mirror launch; false when the plan cannot use it (geometry, or more remaining tiles than the
// launch's first grid slice holds).
// Box buffer size (wave-passes of 64 sixteen-byte units) of k_ray_lin3_pair_mirror_raw for a plan: the smallest that holds the
// boxes of 98 % of the tile pairs (the others go to the general code with the rest list); 4 boxes of nwp KB each set the
// workgroups per CU.
// `permille`: the share of the tile pairs the buffers must hold (980: k_ray_lin3_pair_mirror_raw; 998 with `max_kb` 11:
// k_ray_lin3_pair_mirror_seq, whose two buffers leave room for nearly every box)
int tile_mirror_raw_passes(const void* host_boxes, const void* host_mboxes, const Geom& g, int permille, int max_kb)
{
    const TileBox* b = (const TileBox*)host_boxes;
    const TileBox* q = (const TileBox*)host_mboxes;
    const dim3 d = tile_grid(g, tile_threads(g), 1);
    std::vector<int> hist(kRawMaxWavePasses + 2, 0);
    size_t n = 0;
    for (unsigned ty = 0; ty <= d.y / 2; ty++)
        for (unsigned tx = 0; tx < d.x; tx++) {
            const size_t i = (size_t)ty * d.x + tx;
            if (b[i].cpr <= 0 || q[i].cpr <= 0 || b[i].cpr > kMaxCpr || q[i].cpr > kMaxCpr)
                continue;
            const int u = std::max(b[i].nrows * raw_units_per_row(b[i].cpr), q[i].nrows * raw_units_per_row(q[i].cpr));
            hist[std::min((u + 63) / 64, kRawMaxWavePasses + 1)]++, n++;
        }
    size_t acc = 0;
    for (int k = 0; k <= kRawMaxWavePasses; k++) {
        acc += hist[k];
        if (acc * 1000 >= n * (size_t)permille)
            return std::min(std::max(k, 4), max_kb);
    }
    return max_kb;
}

// `full_rows` (raw_nwp > 0): the list for k_ray_lin3_pair_mirror_raw, whose workgroups serve tile rows 0 .. TY / 2 (mirror_raw_fit) and
// `n_eyes` units; otherwise tile rows 1 .. TY / 2 - 1 pair up and rows 0, TY / 2 and TY - 1 are always on the list
bool tile_mirror_rest(const void* host_boxes, const void* host_mboxes, const Geom& g, int half_dwords, int mirror_h,
                      std::vector<uint32_t>& rest, int raw_nwp, bool full_rows, int n_eyes)
{
    const TileBox* b = (const TileBox*)host_boxes;
    const TileBox* q = (const TileBox*)host_mboxes;
    const dim3 d = tile_grid(g, tile_threads(g), 1);
    rest.clear();
    const int th = tile_threads(g) / kLanesX;  // tile height
    if (mirror_h != g.dst_h || g.dst_h % (2 * th) != 0 || g.dst_w % 4 != 0 || d.x > 0xffffu || d.y > 0xffffu)
        return false;
    const unsigned TY = d.y, TYh = TY / 2;
    if (TYh < 3)
        return false;
    std::vector<uint8_t> in_rest((size_t)d.x * d.y, 0);
    auto add = [&](unsigned tx, unsigned ty) { in_rest[(size_t)ty * d.x + tx] = 1; };
    if (full_rows && raw_nwp > 0) {
        for (unsigned ty = 0; ty <= TYh; ty++)
            for (unsigned tx = 0; tx < d.x; tx++) {
                const size_t i = (size_t)ty * d.x + tx;
                const int fit = mirror_raw_fit(b[i], q[i], raw_nwp, g.src_h, g.src_w);
                if (fit != 1) {
                    add(tx, ty);
                    if (ty < TYh) {  // its band: 15 rows of tile row TY - 1 - ty and (ty > 0) the first row of tile row TY - ty
                        add(tx, TY - 1 - ty);
                        if (ty > 0)
                            add(tx, TY - ty);
                    }
                }
            }
    } else {
        for (unsigned tx = 0; tx < d.x; tx++)
            add(tx, 0), add(tx, TYh), add(tx, TY - 1);
        for (unsigned ty = 1; ty < TYh; ty++)
            for (unsigned tx = 0; tx < d.x; tx++) {
                const size_t i = (size_t)ty * d.x + tx;
                if (raw_nwp > 0 ? !mirror_raw_static_ok(b[i], q[i], raw_nwp, g.src_h, g.src_w) : !mirror_static_ok(b[i], q[i], half_dwords, g.src_h, g.src_w))
                    add(tx, ty), add(tx, TY - 1 - ty), add(tx, TY - ty);
            }
    }
    for (unsigned ty = 0; ty < d.y; ty++)
        for (unsigned tx = 0; tx < d.x; tx++)
            if (in_rest[(size_t)ty * d.x + tx])
                rest.push_back(ty << 16 | tx);
    // worth it only while the mirror path serves most of the image, and the list must fit grid slice 0
    return rest.size() <= (size_t)d.x * (TYh - 1) && rest.size() * 4 <= (size_t)d.x * d.y;
}

void tile_mirror_records(const void* host_boxes, const void* host_mboxes, size_t n_tiles, const Geom& g, int seq_kb, int one_kb, std::vector<char>& out,
                         int tap_s)
{
    const TileBox* b = (const TileBox*)host_boxes;
    const TileBox* q = (const TileBox*)host_mboxes;
    out.resize(n_tiles * sizeof(MirrorRecWords));
    for (size_t i = 0; i < n_tiles; i++) {
        const MirrorRecWords w = mirror_rec_encode(b[i], q[i], seq_kb, one_kb, g.src_h, g.src_w, tap_s);
        std::memcpy(&out[i * sizeof(MirrorRecWords)], &w, sizeof(w));
    }
}

// lu.n = 2: apply_lr's pair; 1 (raw_nwp > 0): a single image through the one-eye instantiation of the LDS-DMA kernel
// seq_kb > 0 (pairs): k_ray_lin3_pair_mirror_seq, two box buffers of seq_kb KB, the eyes one after the other
hipError_t launch_ray_lin3_pair_mirror(const KernelCtx& c, const KernelCtx* cdev, const LaunchUnits& lu, uint32_t* flags, const void* boxes,
                                       const void* mboxes, int half_dwords, int mirror_h, const uint32_t* rest_list, int n_rest, int raw_nwp,
                                       hipStream_t stream, int seq_kb, const void* recs, const void* tap_table, int tap_entry_bytes)
{
    const int n_eyes = lu.n;
    const dim3 full = tile_grid(c.g, 256, 1);
    const dim3 block(256, 1, 1);
    TileArgs a = tile_args(c, cdev, lu, flags);
    a.boxes = (const TileBox*)boxes, a.mboxes = (const TileBox*)mboxes;
    a.rest_list = rest_list, a.n_rest = n_rest;
    a.half_dwords = half_dwords, a.mirror_h = mirror_h;
    a.tiles_x_magic = (unsigned)(0x100000000ull / full.x) + 1u;
    static const unsigned strip_rows = [] {  // V1C_MIRROR_STRIP_ROWS=<n>: A/B override (0: one block per XCD)
        const char* e = tuning_env("V1C_MIRROR_STRIP_ROWS");
        return e ? (unsigned)std::atoi(e) : 2u;
    }();
    static const unsigned block_rows = [] {  // V1C_MIRROR_BLOCK_ROWS=<n>: XCD blocks of gridDim.x / 8 columns x n tile rows (xcd_tile)
        const char* e = tuning_env("V1C_MIRROR_BLOCK_ROWS");
        return e ? (unsigned)std::atoi(e) : 0u;
    }();
    // the LDS-DMA kernels serve tile rows 0 .. TY / 2 (two more than the register-staged pairing of rows 1 .. TY / 2 - 1)
    [[maybe_unused]] auto strips = [&](unsigned rows) {  // two tile rows per strip (tile_xcd_strips): the tuning build's A/B partners
        const unsigned per = (full.x * rows) >> 3;
        unsigned slen = strip_rows && strip_rows * full.x < per ? strip_rows * full.x : 0u;
        if (block_rows && full.x % 8 == 0 && raw_nwp > 0)
            slen = 0x80000000u | std::min(block_rows, 0xffffu);
        a.strip_len = slen;
        a.strip_magic = (slen && !(slen & 0x80000000u)) ? (unsigned)(0x100000000ull / slen) + 1u : 0u;
    };
    const unsigned raw_rows = full.y / 2 + 1;
    const unsigned rest_rows = ((((unsigned)n_rest + full.x - 1) / full.x) + 7u) & ~7u;  // whole rows, a multiple of 8: the pair rows keep their XCDs
    // The LDS-DMA kernels take the head of their arguments as preloaded scalar parameters (V1C_MIRROR_HEAD): the (tile, band) box pairs
    // (`mboxes`), tiles_x | rest_rows << 16, rows of tile pairs | XCD strip rows << 16 (two tile rows per strip, or one block per XCD), the
    // destination size, the base of the plan's row / column tables (= col_s: one buffer), the context, box KB | mirror row << 16
    const unsigned srows = strip_rows == 2u && 2u * full.x < ((full.x * raw_rows) >> 3) ? 2u : 0u;
    const unsigned rows_strip = raw_rows | srows << 16, dst_wh = (unsigned)c.g.dst_w | (unsigned)c.g.dst_h << 16;
    // (`pairs` of the head: the plan's launch records -- MirrorRec, tile_device.hpp -- for the seq and one-eye kernels, the plain box pairs
    // for their A/B partners of the tuning build)
    const TileBox* head_pairs = (const TileBox*)recs;
#define V1C_MIRROR_LAUNCH(KERNEL, GRID, LDS, RESTROWS)                                                                                    \
    hipLaunchKernelGGL(KERNEL, GRID, block, LDS, stream, head_pairs, a.tiles_x_magic, full.x | (unsigned)(RESTROWS) << 16, rows_strip, dst_wh, \
                       a.col_s, a.ctx, (unsigned)a.kb | (unsigned)a.mirror_h << 16, a)
    [[maybe_unused]] bool rec_off = false;
#ifdef V1C_TUNING
    static const bool rec_off_env = [] {  // V1C_MIRROR_REC=0 (A/B): the prologue that decodes the box pair in every wave
        const char* e = tuning_env("V1C_MIRROR_REC");
        return e && e[0] == '0';
    }();
    rec_off = rec_off_env;
#endif
    if (seq_kb > 0 && n_eyes == 2) {  // the eyes one after the other: two buffers of seq_kb KB (rest list made for that size)
        static const bool norest_off = [] {  // V1C_SEQ_NOREST=0 (A/B): the instantiation with the general pair code for every plan
            const char* e = tuning_env("V1C_SEQ_NOREST");
            return e && e[0] == '0';
        }();
        a.kb = seq_kb;
        if (!rec_off && recs == nullptr)
            return hipErrorInvalidValue;
        if (n_rest == 0 && !norest_off) {  // nothing for the general pair code: the instantiation (and the LDS) without it
            const dim3 rgrid(full.x, raw_rows, 1);
            const size_t slds = (size_t)2 * 1024 * (size_t)seq_kb + 16;
            a.rest_rows = 0;
#ifdef V1C_TUNING
            if (rec_off) {
                head_pairs = a.mboxes;
                if (c.ray.var_is_w)
                    V1C_MIRROR_LAUNCH((k_ray_lin3_pair_mirror_seq_box<1, 0>), rgrid, slds, 0u);
                else
                    V1C_MIRROR_LAUNCH((k_ray_lin3_pair_mirror_seq_box<0, 0>), rgrid, slds, 0u);
                return hipGetLastError();
            }
            static const bool tab_off = [] {  // V1C_MIRROR_TAB=0 (A/B): the kernel that evaluates the map, whatever the plan holds
                const char* e = tuning_env("V1C_MIRROR_TAB");
                return e && e[0] == '0';
            }();
            if (tab_off)
                tap_table = nullptr;
#endif
            if (tap_table) {  // the plan's tap table in the head's table slot: the kernel that reads its coordinates, in the plan's entry form
                if (tap_entry_bytes == kTap8EntryBytes)
                    hipLaunchKernelGGL(k_ray_lin3_pair_mirror_seq_tab8, rgrid, block, slds, stream, head_pairs, a.tiles_x_magic, full.x, rows_strip, dst_wh,
                                       (const double*)tap_table, a.ctx, (unsigned)a.kb | (unsigned)a.mirror_h << 16, a);
                else
                    hipLaunchKernelGGL(k_ray_lin3_pair_mirror_seq_tab, rgrid, block, slds, stream, head_pairs, a.tiles_x_magic, full.x, rows_strip, dst_wh,
                                       (const double*)tap_table, a.ctx, (unsigned)a.kb | (unsigned)a.mirror_h << 16, a);
                return hipGetLastError();
            }
            if (c.ray.var_is_w)
                V1C_MIRROR_LAUNCH((k_ray_lin3_pair_mirror_seq<1, 0>), rgrid, slds, 0u);
            else
                V1C_MIRROR_LAUNCH((k_ray_lin3_pair_mirror_seq<0, 0>), rgrid, slds, 0u);
            return hipGetLastError();
        }
        const dim3 rgrid(full.x, raw_rows + rest_rows, 1);
        const size_t slds = std::max((size_t)half_dwords * 8 + 16, (size_t)2 * 1024 * (size_t)seq_kb);
        a.rest_rows = rest_rows;
#ifdef V1C_TUNING
        if (rec_off) {
            head_pairs = a.mboxes;
            if (c.ray.var_is_w)
                V1C_MIRROR_LAUNCH((k_ray_lin3_pair_mirror_seq_box<1>), rgrid, slds, rest_rows);
            else
                V1C_MIRROR_LAUNCH((k_ray_lin3_pair_mirror_seq_box<0>), rgrid, slds, rest_rows);
            return hipGetLastError();
        }
#endif
        if (c.ray.var_is_w)
            V1C_MIRROR_LAUNCH((k_ray_lin3_pair_mirror_seq<1>), rgrid, slds, rest_rows);
        else
            V1C_MIRROR_LAUNCH((k_ray_lin3_pair_mirror_seq<0>), rgrid, slds, rest_rows);
        return hipGetLastError();
    }
    if (raw_nwp > 0 && n_eyes == 1) {  // a single image: the LDS-DMA kernel's one-eye instantiation
        const dim3 rgrid(full.x, raw_rows + rest_rows, 1);
        // two boxes; the general pair code serves one unit from one cell buffer
        const size_t lds = std::max((size_t)half_dwords * 4 + 16, (size_t)2 * 1024 * (size_t)raw_nwp);
        a.kb = raw_nwp, a.rest_rows = rest_rows;
        if (!rec_off && recs == nullptr)
            return hipErrorInvalidValue;
#ifdef V1C_TUNING
        if (rec_off) {
            head_pairs = a.mboxes;
            if (c.ray.var_is_w)
                V1C_MIRROR_LAUNCH((k_ray_lin3_pair_mirror_box_raw<1>), rgrid, lds, rest_rows);
            else
                V1C_MIRROR_LAUNCH((k_ray_lin3_pair_mirror_box_raw<0>), rgrid, lds, rest_rows);
            return hipGetLastError();
        }
#endif
        if (c.ray.var_is_w)
            V1C_MIRROR_LAUNCH((k_ray_lin3_pair_mirror_raw<1, 1>), rgrid, lds, rest_rows);
        else
            V1C_MIRROR_LAUNCH((k_ray_lin3_pair_mirror_raw<0, 1>), rgrid, lds, rest_rows);
        return hipGetLastError();
    }
#ifdef V1C_TUNING  // A/B partners of the seq kernel: the four-buffer LDS-DMA pair kernel (V1C_MIRROR_SEQ=0) and the register-staged one (V1C_MIRROR_RAW=0)
    if (n_eyes != 2)
        return hipErrorInvalidValue;
    const size_t lds = std::max((size_t)half_dwords * 8 + 16, (size_t)4 * 1024 * (size_t)std::max(raw_nwp, 0));
    if (raw_nwp > 0) {
        dim3 rgrid(full.x, raw_rows + rest_rows, 1);
        strips(raw_rows);
        a.kb = raw_nwp, a.rest_rows = rest_rows;
        // V1C_MIRROR_SKIP=1: timing experiment, the rest rows are not launched (their tiles stay unwritten); =2: ONLY the rest rows
        static const int skip = [] {
            const char* e = tuning_env("V1C_MIRROR_SKIP");
            return e ? std::atoi(e) : 0;
        }();
        if (skip == 1)
            a.n_rest = 0, a.rest_rows = 0, rgrid.y = raw_rows;
        if (skip == 2)
            rgrid.y = rest_rows;
        const unsigned rr = skip == 1 ? 0u : rest_rows;
        head_pairs = a.mboxes;
        if (c.ray.var_is_w)
            V1C_MIRROR_LAUNCH((k_ray_lin3_pair_mirror_raw<1, 2>), rgrid, lds, rr);
        else
            V1C_MIRROR_LAUNCH((k_ray_lin3_pair_mirror_raw<0, 2>), rgrid, lds, rr);
        return hipGetLastError();
    }
    const dim3 grid(full.x, full.y / 2 - 1, 2);
    strips(grid.y);
    if (c.ray.var_is_w)
        hipLaunchKernelGGL((k_ray_lin3_pair_mirror<1>), grid, block, lds, stream, a);
    else
        hipLaunchKernelGGL((k_ray_lin3_pair_mirror<0>), grid, block, lds, stream, a);
    return hipGetLastError();
#else
    return hipErrorInvalidValue;  // (plan.hip selects the seq / one-eye forms only)
#endif
}

}  // namespace v1c
