// kernels_feat.hip -- the device side of v1c_feat_detect / v1c_feat_match (feat.hip): luma + block resampling, binomial smoothing,
// FAST-9 scores, non-maximum suppression and per-cell selection, the N_max cap, orientation + steered binary descriptors, and the
// brute-force Hamming matcher.  A code object of its own: a process that only remaps images never loads these kernels.
//
// wave64 throughout; every kernel does a bounded amount of work per lane and waits on nothing but its own workgroup's barriers.  The
// arithmetic is feat_core.hpp's; the order of every list is fixed by the data, never by the order in which atomics land.
#include "feat_launch.hpp"

namespace v1c {
namespace feat {

constexpr int kTileW = 64, kTileH = 16;  // smoothing tile: outputs per workgroup, plus a 2-pixel halo on every side

// stage 1: working pixel (x, y) = round-half-up mean of the luma of its source block
__global__ __launch_bounds__(256) void k_feat_luma(DetectArgs a)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= a.ww || y >= a.wh)
        return;
    const int r0 = a.rb[y], r1 = a.rb[y + 1], c0 = a.cb[x], c1 = a.cb[x + 1];
    int sum = 0;
    for (int r = r0; r < r1; r++) {
        const uint8_t* row = a.src + (int64_t)r * a.pitch;
        for (int c = c0; c < c1; c++)
            sum += luma(row + (int64_t)c * a.cn, a.cn);
    }
    a.y[(int64_t)y * a.ww + x] = (uint8_t)block_mean(sum, (r1 - r0) * (c1 - c0));
}

// stage 2: [1 4 6 4 1] horizontally, then vertically, each pass rounded; the border replicated.  The tile and its halo go through
// LDS once: rows y0 - 2 .. y0 + kTileH + 1 and columns x0 - 2 .. x0 + kTileW + 1, clamped to the image.
__global__ __launch_bounds__(256) void k_feat_smooth(DetectArgs a)
{
    __shared__ int raw[kTileH + 4][kTileW + 4];
    __shared__ int hor[kTileH + 4][kTileW];
    const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH, t = threadIdx.x;
    for (int i = t; i < (kTileH + 4) * (kTileW + 4); i += 256) {
        const int ly = i / (kTileW + 4), lx = i % (kTileW + 4);
        const int gy = min(max(y0 + ly - 2, 0), a.wh - 1), gx = min(max(x0 + lx - 2, 0), a.ww - 1);
        raw[ly][lx] = a.y[(int64_t)gy * a.ww + gx];
    }
    __syncthreads();
    for (int i = t; i < (kTileH + 4) * kTileW; i += 256) {
        const int ly = i / kTileW, lx = i % kTileW;
        hor[ly][lx] = smooth5(raw[ly][lx], raw[ly][lx + 1], raw[ly][lx + 2], raw[ly][lx + 3], raw[ly][lx + 4]);
    }
    __syncthreads();
    for (int i = t; i < kTileH * kTileW; i += 256) {
        const int ly = i / kTileW, lx = i % kTileW, gx = x0 + lx, gy = y0 + ly;
        if (gx < a.ww && gy < a.wh)
            a.sm[(int64_t)gy * a.ww + gx] =
                (uint8_t)smooth5(hor[ly][lx], hor[ly + 1][lx], hor[ly + 2][lx], hor[ly + 3][lx], hor[ly + 4][lx]);
    }
}

// stage 3: candidate score map of the unsmoothed luma -- the FAST-9 score where it reaches the threshold inside the qualifying disc
// (the host's per-row column ranges, empty in the kBorder rows next to the top and bottom edges and never reaching the kBorder
// columns next to the left and right ones: FAST, NMS and the descriptor disc then read inside the image), 0 everywhere else
__global__ __launch_bounds__(256) void k_feat_fast(DetectArgs a)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= a.ww || y >= a.wh)
        return;
    int s = 0;
    if (x >= a.rng[2 * y] && x <= a.rng[2 * y + 1]) {
        const int f = fast_score(a.y, a.ww, x, y);
        s = f >= a.threshold ? f : 0;
    }
    a.score[(int64_t)y * a.ww + x] = (uint8_t)s;
}

__device__ inline uint32_t wave_max(uint32_t v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = __shfl_xor(v, off);
        v = o > v ? o : v;
    }
    return v;
}

// stage 4a: one workgroup per grid cell -- the NMS survivors of the cell, the best `per_cell` of them by (score desc, y, x) as ranking
// keys in slots cell * per_cell + rank (0 = empty slot), and their scores counted into the histogram of the N_max cap
__global__ __launch_bounds__(256) void k_feat_select(DetectArgs a, int ncx)
{
    constexpr int kPx = kMaxCell * kMaxCell / 256;
    const int cell = blockIdx.x, cs = a.cell;
    const int cx0 = (cell % ncx) * cs, cy0 = (cell / ncx) * cs;
    uint32_t keys[kPx];
#pragma unroll
    for (int i = 0; i < kPx; i++) {
        const int p = threadIdx.x + 256 * i;
        uint32_t key = 0;
        if (p < cs * cs) {
            const int x = cx0 + p % cs, y = cy0 + p / cs;
            if (x < a.ww && y < a.wh) {
                const int s = a.score[(int64_t)y * a.ww + x];
                if (s > 0 && nms_keep(a.score, a.ww, x, y))
                    key = cell_key(s, p);
            }
        }
        keys[i] = key;
    }
    __shared__ uint32_t red[4];
    uint32_t prev = 0xffffffffu;
    for (int r = 0; r < a.per_cell; r++) {
        uint32_t m = 0;
#pragma unroll
        for (int i = 0; i < kPx; i++)
            m = keys[i] < prev && keys[i] > m ? keys[i] : m;
        m = wave_max(m);
        if ((threadIdx.x & 63) == 0)
            red[threadIdx.x >> 6] = m;
        __syncthreads();
        m = max(max(red[0], red[1]), max(red[2], red[3]));
        __syncthreads();
        if (threadIdx.x == 0) {
            a.cand[(int64_t)cell * a.per_cell + r] = m;
            if (m)
                atomicAdd(&a.hist[key_score(m)], 1u);
        }
        prev = m;
    }
}

// exclusive prefix sum over a 1024-lane workgroup; *total = the sum of all lanes
__device__ inline int block_scan_1024(int v, int* total)
{
    __shared__ int ws[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int n = __shfl_up(inc, off);
        if (lane >= off)
            inc += n;
    }
    if (lane == 63)
        ws[wave] = inc;
    __syncthreads();
    int base = 0, tot = 0;
    for (int k = 0; k < 16; k++) {
        const int c = ws[k];
        base += k < wave ? c : 0;
        tot += c;
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

// stage 4b (one workgroup of 1024): the N_max cap and the compaction.  From the score histogram: the lowest kept score T and the
// quota of slots with score == T -- all slots above T are kept, and the first `quota` at T in slot order, i.e. in the order
// (score desc, cell index, rank in cell).  The kept slots are written in slot order: the list is cell-major.  Each lane walks its own
// contiguous range of slots, three times.
__global__ __launch_bounds__(1024) void k_feat_compact(DetectArgs a, int nslots)
{
    __shared__ int s_thr[2];
    if (threadIdx.x == 0) {
        int acc = 0, thr = 0, quota = 0;
        for (int s = 255; s >= 1; s--) {
            const int n = (int)a.hist[s];
            if (acc + n >= a.max_kp) {
                thr = s;
                quota = a.max_kp - acc;
                break;
            }
            acc += n;
        }
        s_thr[0] = thr;
        s_thr[1] = quota;
    }
    __syncthreads();
    const int thr = s_thr[0], quota = s_thr[1];
    const int seg = (nslots + 1023) / 1024;
    const int b0 = min(nslots, (int)threadIdx.x * seg), b1 = min(nslots, b0 + seg);
    int n_eq = 0;
    for (int i = b0; i < b1; i++)
        n_eq += a.cand[i] && key_score(a.cand[i]) == thr;
    int total;
    const int eq_before = block_scan_1024(n_eq, &total);
    int n_kept = 0;
    for (int i = b0, e = eq_before; i < b1; i++) {
        const uint32_t k = a.cand[i];
        const int s = key_score(k);
        n_kept += k && (s > thr || (s == thr && e < quota));
        e += k && s == thr;
    }
    const int out_before = block_scan_1024(n_kept, &total);
    const int ncx = (a.ww + a.cell - 1) / a.cell;
    int o = out_before;
    for (int i = b0, e = eq_before; i < b1; i++) {
        const uint32_t k = a.cand[i];
        const int s = key_score(k);
        const bool keep = k && (s > thr || (s == thr && e < quota));
        e += k && s == thr;
        if (!keep || o >= a.max_kp)
            continue;
        const int cell = i / a.per_cell, p = key_pixel(k);
        const int x = (cell % ncx) * a.cell + p % a.cell, y = (cell / ncx) * a.cell + p / a.cell;
        Kp r;
        r.x = x;
        r.y = y;
        r.score = s;
        r.bin = 0;
        r.src_x2 = a.cb[x] + a.cb[x + 1] - 1;
        r.src_y2 = a.rb[y] + a.rb[y + 1] - 1;
        a.kp[o++] = r;
    }
    if (threadIdx.x == 0)
        *a.count = min(total, a.max_kp);
}

// stage 5: one wave per keypoint -- the moments of the radius-15 disc of the smoothed image, the orientation sector, and the 256
// bits I(p_b) < I(q_b) of the sector's rotated pattern, 64 per ballot
__global__ __launch_bounds__(256) void k_feat_describe(DetectArgs a)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= *a.count)
        return;
    const int x = a.kp[i].x, y = a.kp[i].y;
    const uint8_t* c = a.sm + (int64_t)y * a.ww + x;
    int m10 = 0, m01 = 0;
    constexpr int kSquare = (2 * kPatchRadius + 1) * (2 * kPatchRadius + 1);
    for (int q = lane; q < kSquare; q += 64) {
        int dx, dy;
        if (disc_offset(q, &dx, &dy)) {
            const int v = c[(int64_t)dy * a.ww + dx];
            m10 += dx * v;
            m01 += dy * v;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        m10 += __shfl_xor(m10, off);
        m01 += __shfl_xor(m01, off);
    }
    const int bin = orient_bin(m10, m01, a.bv);
    uint64_t words[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int8_t* e = a.pattern + ((int64_t)bin * kPairs + j * 64 + lane) * 4;
        const bool bit = c[(int64_t)e[1] * a.ww + e[0]] < c[(int64_t)e[3] * a.ww + e[2]];
        words[j] = __ballot(bit);
    }
    if (lane == 0) {
        uint64_t* d = (uint64_t*)(a.desc + (int64_t)i * kDescBytes);
#pragma unroll
        for (int j = 0; j < 4; j++)
            d[j] = words[j];
        a.kp[i].bin = bin;
    }
}

hipError_t launch_detect(const DetectArgs& a, hipStream_t st)
{
    const dim3 px((a.ww + 63) / 64, (a.wh + 3) / 4), b64x4(64, 4);
    const int ncx = (a.ww + a.cell - 1) / a.cell, ncy = (a.wh + a.cell - 1) / a.cell;
    hipLaunchKernelGGL(k_feat_luma, px, b64x4, 0, st, a);
    hipLaunchKernelGGL(k_feat_smooth, dim3((a.ww + kTileW - 1) / kTileW, (a.wh + kTileH - 1) / kTileH), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_feat_fast, px, b64x4, 0, st, a);
    hipLaunchKernelGGL(k_feat_select, dim3(ncx * ncy), dim3(256), 0, st, a, ncx);
    hipLaunchKernelGGL(k_feat_compact, dim3(1), dim3(1024), 0, st, a, ncx * ncy * a.per_cell);
    hipLaunchKernelGGL(k_feat_describe, dim3((a.max_kp + 3) / 4), dim3(256), 0, st, a);
    return hipGetLastError();
}

// ---- matcher ---------------------------------------------------------------------------------------------------------------------

constexpr int kMatchBlock = 256;  // queries per workgroup (one per lane) = candidates per LDS tile

// partial best of every query over one chunk of candidates: the chunk streams through LDS in tiles of 256 descriptors, stored as two
// planes of 16-byte halves so that the tile fill is conflict-free; every lane reads the same row (a broadcast ds_read_b128 pair)
__global__ __launch_bounds__(kMatchBlock) void k_feat_best(const uint8_t* q, int nq, const uint8_t* t, int nt, int chunk, Best* part)
{
    __shared__ uint4 lo[kMatchBlock], hi[kMatchBlock];
    const int i = blockIdx.x * kMatchBlock + threadIdx.x;
    uint4 qa = make_uint4(0, 0, 0, 0), qb = qa;
    if (i < nq) {
        const uint4* p = (const uint4*)(q + (int64_t)i * kDescBytes);
        qa = p[0];
        qb = p[1];
    }
    Best b = best_init();
    const int j0 = blockIdx.y * chunk, j1 = min(nt, j0 + chunk);
    for (int t0 = j0; t0 < j1; t0 += kMatchBlock) {
        const int n = min(kMatchBlock, j1 - t0);
        __syncthreads();
        if ((int)threadIdx.x < n) {
            const uint4* p = (const uint4*)(t + (int64_t)(t0 + threadIdx.x) * kDescBytes);
            lo[threadIdx.x] = p[0];
            hi[threadIdx.x] = p[1];
        }
        __syncthreads();
        for (int j = 0; j < n; j++) {
            const uint4 u = lo[j], v = hi[j];
            const int d = __popc(qa.x ^ u.x) + __popc(qa.y ^ u.y) + __popc(qa.z ^ u.z) + __popc(qa.w ^ u.w) + __popc(qb.x ^ v.x) +
                          __popc(qb.y ^ v.y) + __popc(qb.z ^ v.z) + __popc(qb.w ^ v.w);
            best_push(b, d, t0 + j);
        }
    }
    if (i < nq)
        part[(int64_t)blockIdx.y * nq + i] = b;
}

// the chunks' partial results of every query, merged in chunk order (ties keep the lower index)
__global__ __launch_bounds__(256) void k_feat_merge(const Best* part, int nch, int nq, Best* best)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nq)
        return;
    Best b = part[i];
    for (int c = 1; c < nch; c++)
        b = best_merge(b, part[(int64_t)c * nq + i]);
    best[i] = b;
}

// the kept pairs in query order (one workgroup of 1024, each lane a contiguous range of queries, twice)
__global__ __launch_bounds__(1024) void k_feat_pairs(const Best* ab, int n_a, const Best* ba, int d_max, int num, int den,
                                                     int32_t* pairs, int32_t* dist, int32_t* count)
{
    const int seg = (n_a + 1023) / 1024;
    const int b0 = min(n_a, (int)threadIdx.x * seg), b1 = min(n_a, b0 + seg);
    int n = 0;
    for (int i = b0; i < b1; i++)
        n += match_keep(ab[i], ba[ab[i].idx], i, d_max, num, den);
    int total;
    int o = block_scan_1024(n, &total);
    for (int i = b0; i < b1; i++) {
        const Best bi = ab[i];
        if (!match_keep(bi, ba[bi.idx], i, d_max, num, den))
            continue;
        pairs[2 * o] = i;
        pairs[2 * o + 1] = bi.idx;
        dist[o] = bi.d1;
        o++;
    }
    if (threadIdx.x == 0)
        *count = total;
}

// chunking of the candidates: enough workgroups to fill the GPU when the query set is small, at most 64 partial results per query
static void match_plan(int nq, int nt, int* nch, int* chunk)
{
    const int qblocks = (nq + kMatchBlock - 1) / kMatchBlock;
    int n = (nt + kMatchBlock - 1) / kMatchBlock;
    n = min(n, max(1, (2048 + qblocks - 1) / qblocks));
    n = min(n, 64);
    const int per = (nt + n - 1) / n;
    *chunk = (per + kMatchBlock - 1) / kMatchBlock * kMatchBlock;
    *nch = (nt + *chunk - 1) / *chunk;
}

size_t match_scratch_bytes(int n_a, int n_b)
{
    int nch_a, nch_b, c;
    match_plan(n_a, n_b, &nch_b, &c);
    match_plan(n_b, n_a, &nch_a, &c);
    return sizeof(Best) * ((size_t)nch_b * n_a + (size_t)nch_a * n_b + n_a + n_b);
}

hipError_t launch_match(const uint8_t* da, int n_a, const uint8_t* db, int n_b, int d_max, int num, int den, void* scratch,
                        int32_t* pairs, int32_t* dist, int32_t* count, hipStream_t st)
{
    int nch_a, nch_b, chunk_a, chunk_b;
    match_plan(n_a, n_b, &nch_b, &chunk_b);
    match_plan(n_b, n_a, &nch_a, &chunk_a);
    Best* part_ab = (Best*)scratch;
    Best* part_ba = part_ab + (size_t)nch_b * n_a;
    Best* best_ab = part_ba + (size_t)nch_a * n_b;
    Best* best_ba = best_ab + n_a;
    hipLaunchKernelGGL(k_feat_best, dim3((n_a + kMatchBlock - 1) / kMatchBlock, nch_b), dim3(kMatchBlock), 0, st, da, n_a, db, n_b,
                       chunk_b, part_ab);
    hipLaunchKernelGGL(k_feat_best, dim3((n_b + kMatchBlock - 1) / kMatchBlock, nch_a), dim3(kMatchBlock), 0, st, db, n_b, da, n_a,
                       chunk_a, part_ba);
    hipLaunchKernelGGL(k_feat_merge, dim3((n_a + 255) / 256), dim3(256), 0, st, part_ab, nch_b, n_a, best_ab);
    hipLaunchKernelGGL(k_feat_merge, dim3((n_b + 255) / 256), dim3(256), 0, st, part_ba, nch_a, n_b, best_ba);
    hipLaunchKernelGGL(k_feat_pairs, dim3(1), dim3(1024), 0, st, best_ab, n_a, best_ba, d_max, num, den, pairs, dist, count);
    return hipGetLastError();
}

}  // namespace feat
}  // namespace v1c
