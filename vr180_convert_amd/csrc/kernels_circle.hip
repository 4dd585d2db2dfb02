// kernels_circle.hip -- the image-circle fit on the device: rim points of every row and
// every column, then the trimmed algebraic fit of one workgroup.  A code object of its own; the arithmetic is circle_core.hpp's.
//   k_circle_rows       one wave per row: steps of 64 pixels, eight in flight, from the left until the run is found, then from the right
//   k_circle_col_bands  one wave per strip of 64 columns (lane = column) and band of 64 rows: the band's record of every column
//   k_circle_col_join   lane = column: down and up through the column's band records to its two points
//   k_circle_fit        one workgroup: selection, integer moment sums (wave shuffles, then LDS), the solve by one lane, every round
// A column walked from its top to its run by ONE wave is a chain of dependent loads as long as the black border is high (1.1 ms of a
// 1.3 ms fit on a 4096 x 4096 disc); cut into bands the columns cost one read of the image, by as many waves as
// there are strips x bands.
#include <hip/hip_runtime.h>

#include "circle_launch.hpp"

namespace v1c {
namespace circle {

namespace {

constexpr int kRowsPerBlock = 4;   // waves of a rows block
constexpr int kColBatch = 16;      // rows a column wave has in flight
constexpr int kRowSteps = 16;      // 64-pixel steps a row wave has in flight
constexpr int kJoinBatch = 16;     // band records a joining lane has in flight
constexpr int kFitBatch = 8;       // points a fitting thread has in flight
constexpr int kFitCache = 32768;   // point slots the fit keeps in LDS after its first pass (128 KiB: 2 (h + w) of an 8192 x 8192 frame)
constexpr int kFitThreads = 512;
constexpr int kFitWaves = kFitThreads / 64;

// channel sum of pixel x of a row
template <typename T, int CN>
__device__ __forceinline__ int pixel_sum(const T* __restrict__ row, int x)
{
    const T* p = row + (int64_t)x * CN;
    int s = p[0];
    if (CN >= 3)
        s += (int)p[1] + (int)p[2];
    if (CN == 4)
        s += p[3];
    return s;
}

// the run search of one row from one end: `REV` scans pixel w - 1 - d at distance d.  Returns the distance of the run's first pixel
// from that end, -1 where the row has no run.
template <typename T, int CN, bool REV>
__device__ __forceinline__ int scan_row(const T* __restrict__ row, int w, int thr_cn, int run, int lane)
{
    uint64_t pm = 0;
    for (int d0 = 0; d0 < w; d0 += 64 * kRowSteps) {
        int s[kRowSteps];
#pragma unroll
        for (int u = 0; u < kRowSteps; u++) {
            const int d = d0 + 64 * u + lane;
            s[u] = d < w ? pixel_sum<T, CN>(row, REV ? w - 1 - d : d) : -1;  // (-1: below every threshold)
        }
#pragma unroll
        for (int u = 0; u < kRowSteps; u++) {
            const uint64_t m = __ballot(s[u] >= thr_cn);
            const uint64_t t = run_ends(m, pm, run);
            if (t)
                return d0 + 64 * u + ctz64(t) - run + 1;
            pm = m;
        }
    }
    return -1;
}

template <typename T, int CN>
__global__ __launch_bounds__(64 * kRowsPerBlock) void k_circle_rows(const uint8_t* __restrict__ img, int64_t pitch, int h, int w, int thr_cn,
                                                                    int run, uint32_t* __restrict__ pts)
{
    const int lane = threadIdx.x & 63;
    const int y = blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
    if (y >= h)
        return;
    const T* row = (const T*)(img + (int64_t)y * pitch);
    int xl = scan_row<T, CN, false>(row, w, thr_cn, run, lane), xr = -1;
    if (xl >= 0)
        xr = w - 1 - scan_row<T, CN, true>(row, w, thr_cn, run, lane);
    if (lane == 0) {
        // a point on the frame's own first or last column is the frame, not the rim
        pts[2 * y] = xl > 0 && xl < w - 1 ? pack_point(xl, y) : kNoPoint;
        pts[2 * y + 1] = xr > 0 && xr < w - 1 ? pack_point(xr, y) : kNoPoint;
    }
}

// the record of one band of one strip of columns: blockIdx.x = strip, blockIdx.y = band
template <typename T, int CN>
__global__ __launch_bounds__(64) void k_circle_col_bands(const uint8_t* __restrict__ img, int64_t pitch, int h, int w, int thr_cn, int run,
                                                         uint32_t* __restrict__ rec)
{
    const int x = blockIdx.x * 64 + threadIdx.x;
    const int xc = x < w ? x : w - 1;
    const int y0 = blockIdx.y * kBandRows;
    const int rows = h - y0 < kBandRows ? h - y0 : kBandRows;
    BandScan b;
    for (int o0 = 0; o0 < rows; o0 += kColBatch) {
        int s[kColBatch];
#pragma unroll
        for (int u = 0; u < kColBatch; u++)
            s[u] = o0 + u < rows ? pixel_sum<T, CN>((const T*)(img + (int64_t)(y0 + o0 + u) * pitch), xc) : -1;
#pragma unroll
        for (int u = 0; u < kColBatch; u++)
            if (o0 + u < rows)
                band_step(b, s[u] >= thr_cn, o0 + u, run);
    }
    if (x < w)
        rec[(size_t)blockIdx.y * w + x] = band_pack(b, rows);
}

// a column's two points from its band records
__global__ __launch_bounds__(64) void k_circle_col_join(const uint32_t* __restrict__ rec, int h, int w, int run, uint32_t* __restrict__ pts)
{
    const int x = blockIdx.x * 64 + threadIdx.x;
    if (x >= w)
        return;
    const int nb = (h + kBandRows - 1) / kBandRows;
    const int last_rows = h - (nb - 1) * kBandRows;
    ColJoin down, up;
    for (int b0 = 0; b0 < nb && down.found < 0; b0 += kJoinBatch) {
        uint32_t r[kJoinBatch];
#pragma unroll
        for (int u = 0; u < kJoinBatch; u++)
            r[u] = b0 + u < nb ? rec[(size_t)(b0 + u) * w + x] : 0;
#pragma unroll
        for (int u = 0; u < kJoinBatch; u++)
            if (b0 + u < nb)
                join_step(down, r[u], (b0 + u) * kBandRows, b0 + u == nb - 1 ? last_rows : kBandRows, run, true);
    }
    for (int b0 = 0; b0 < nb && up.found < 0 && down.found >= 0; b0 += kJoinBatch) {
        uint32_t r[kJoinBatch];
#pragma unroll
        for (int u = 0; u < kJoinBatch; u++)
            r[u] = b0 + u < nb ? rec[(size_t)(nb - 1 - b0 - u) * w + x] : 0;
#pragma unroll
        for (int u = 0; u < kJoinBatch; u++)
            if (b0 + u < nb)
                join_step(up, r[u], (nb - 1 - b0 - u) * kBandRows, b0 + u == 0 ? last_rows : kBandRows, run, false);
    }
    const int yt = down.found, yb = up.found;
    uint32_t* o = pts + 2 * (size_t)h + 2 * (size_t)x;
    o[0] = yt > 0 && yt < h - 1 ? pack_point(x, yt) : kNoPoint;
    o[1] = yb > 0 && yb < h - 1 ? pack_point(x, yb) : kNoPoint;
}

__device__ __forceinline__ int64_t wave_sum(int64_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        v += __shfl_xor((long long)v, o, 64);
    return v;
}

// sums of the workgroup in every thread of wave 0's lane 0 (thread 0); `part` is free again after the caller's next barrier
template <int N>
__device__ __forceinline__ void block_sums(int64_t (&a)[N], int64_t (*part)[kSums + 1])
{
#pragma unroll
    for (int k = 0; k < N; k++)
        a[k] = wave_sum(a[k]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < N; k++)
            part[threadIdx.x >> 6][k] = a[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < N; k++) {
            int64_t t = 0;
            for (int v = 0; v < kFitWaves; v++)
                t += part[v][k];
            a[k] = t;
        }
    }
}

__global__ __launch_bounds__(kFitThreads) void k_circle_fit(const uint32_t* __restrict__ pts, uint8_t* __restrict__ sel, int n_slots, int h, int w,
                                                            Params prm, double* __restrict__ out)
{
    __shared__ int64_t part[kFitWaves][kSums + 1];
    __shared__ int64_t bc[4];  // status, cx16, cy16, r16 of the fit the next selection uses
    __shared__ uint32_t cache[kFitCache];  // the first slots, read from memory once
    const int tid = threadIdx.x;
    const int x0 = w / 2, y0 = h / 2;
    int64_t cx16 = 0, cy16 = 0, r16 = 0;
    int status = 0;
    // thread 0 alone keeps the result
    Fit f{0.0, 0.0, 0.0, 0};
    int64_t n_rim = 0, n_used = 0;
    for (int round = -1; round < prm.rounds; round++) {
        const int64_t t16 = round >= 0 ? prm.tol16[round] : 0;
        int64_t a[kSums] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int i0 = tid; i0 < n_slots; i0 += kFitThreads * kFitBatch) {
            uint32_t pb[kFitBatch];
#pragma unroll
            for (int u = 0; u < kFitBatch; u++) {
                const int i = i0 + u * kFitThreads;
                pb[u] = i >= n_slots ? kNoPoint : round >= 0 && i < kFitCache ? cache[i] : pts[i];
                if (round < 0 && i < kFitCache && i < n_slots)
                    cache[i] = pb[u];  // (read back by this very thread alone)
            }
#pragma unroll
            for (int u = 0; u < kFitBatch; u++) {
                const int i = i0 + u * kFitThreads;
                const uint32_t p = pb[u];
                bool in = p != kNoPoint;
                const int x = (int)(p & 0xFFFFu) - x0, y = (int)(p >> 16) - y0;
                if (in && round >= 0)
                    in = selected(dist2_16(x, y, cx16, cy16), r16, t16);
                if (i < n_slots)
                    sel[i] = in ? 1 : 0;
                if (in) {
                    const int xx = x * x, yy = y * y, z = xx + yy;
                    a[0] += 1;
                    a[1] += x;
                    a[2] += y;
                    a[3] += xx;
                    a[4] += (int64_t)x * y;
                    a[5] += yy;
                    a[6] += (int64_t)x * z;
                    a[7] += (int64_t)y * z;
                    a[8] += z;
                }
            }
        }
        block_sums<kSums>(a, part);
        if (tid == 0) {
            if (round < 0)
                n_rim = a[0];
            n_used = a[0];
            if (a[0] < prm.min_points)
                f = Fit{0.0, 0.0, 0.0, 1};
            else
                f = solve(a, h, w);
            bc[0] = f.status;
            bc[1] = q16(f.cx);
            bc[2] = q16(f.cy);
            bc[3] = q16(f.r);
        }
        __syncthreads();
        status = (int)bc[0];
        cx16 = bc[1];
        cy16 = bc[2];
        r16 = bc[3];
        if (status)
            break;
    }
    // the quantised residuals of the points of the last selection about the final circle
    int64_t e[1] = {0};
    if (!status) {
        for (int i = tid; i < n_slots; i += kFitThreads) {
            if (sel[i]) {  // (this thread's own store)
                const uint32_t p = i < kFitCache ? cache[i] : pts[i];
                const int64_t d = isqrt64(dist2_16((int)(p & 0xFFFFu) - x0, (int)(p >> 16) - y0, cx16, cy16)) - r16;
                e[0] += d * d;
            }
        }
    }
    block_sums<1>(e, part);
    if (tid == 0) {
        out[0] = status ? 0.0 : (double)x0 + f.cx;
        out[1] = status ? 0.0 : (double)y0 + f.cy;
        out[2] = status ? 0.0 : f.r;
        out[3] = (double)status;
        out[4] = (double)n_rim;
        out[5] = (double)n_used;
        out[6] = status ? 0.0 : rms16(e[0], n_used);
        out[7] = 0.0;
    }
}

template <typename T>
hipError_t launch_scans(const uint8_t* img, int h, int w, int64_t pitch, int cn, int thr_cn, int run, uint32_t* pts, uint32_t* rec, hipStream_t st)
{
    const dim3 gr((h + kRowsPerBlock - 1) / kRowsPerBlock), br(64 * kRowsPerBlock), gc((w + 63) / 64, bands(h)), bcols(64);
    if (cn == 1) {
        hipLaunchKernelGGL((k_circle_rows<T, 1>), gr, br, 0, st, img, pitch, h, w, thr_cn, run, pts);
        hipLaunchKernelGGL((k_circle_col_bands<T, 1>), gc, bcols, 0, st, img, pitch, h, w, thr_cn, run, rec);
    } else if (cn == 3) {
        hipLaunchKernelGGL((k_circle_rows<T, 3>), gr, br, 0, st, img, pitch, h, w, thr_cn, run, pts);
        hipLaunchKernelGGL((k_circle_col_bands<T, 3>), gc, bcols, 0, st, img, pitch, h, w, thr_cn, run, rec);
    } else {
        hipLaunchKernelGGL((k_circle_rows<T, 4>), gr, br, 0, st, img, pitch, h, w, thr_cn, run, pts);
        hipLaunchKernelGGL((k_circle_col_bands<T, 4>), gc, bcols, 0, st, img, pitch, h, w, thr_cn, run, rec);
    }
    hipLaunchKernelGGL(k_circle_col_join, dim3((w + 63) / 64), bcols, 0, st, (const uint32_t*)rec, h, w, run, pts);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_fit(const uint8_t* img, int h, int w, int64_t pitch, int cn, bool depth16, const Params& prm, uint8_t* workspace,
                      double* out8, hipStream_t st)
{
    uint32_t* pts = (uint32_t*)workspace;
    uint8_t* sel = workspace + flags_offset(h, w);
    const int thr_cn = prm.threshold * cn;
    uint32_t* rec = (uint32_t*)(workspace + bands_offset(h, w));
    hipError_t e = depth16 ? launch_scans<uint16_t>(img, h, w, pitch, cn, thr_cn, prm.run, pts, rec, st)
                           : launch_scans<uint8_t>(img, h, w, pitch, cn, thr_cn, prm.run, pts, rec, st);
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(k_circle_fit, dim3(1), dim3(kFitThreads), 0, st, (const uint32_t*)pts, sel, (int)slots(h, w), h, w, prm, out8);
    return hipGetLastError();
}

}  // namespace circle
}  // namespace v1c
