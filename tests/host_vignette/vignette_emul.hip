// vignette_emul.hip -- host build of the vignetting correction: vignette_core.hpp as the kernels compile it, driven through the kernels'
// decomposition (kernels_vignette.hip) -- the rows as items of a grid of `blocks` x 256 threads; in the ring statistics every thread
// with its run, every wave with its own 32-BIT copy of the record, the copies of a workgroup summed and cleared every kFlushItems
// items (an overflow of a copy would show exactly as on the device); the gain pass over the same items, a segment read whole before
// it is written.  Built as a shared library for tests/test_vignette_host.py and, with -DVIGNETTE_MAIN, as a program of its own that the
// sanitizers run over the cases.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../vr180_convert_amd/csrc/vignette_core.hpp"

using namespace v1c::vignette;

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

template <class T>
uint32_t rd(const uint8_t* p)
{
    T v;
    std::memcpy(&v, p, sizeof(T));
    return v;
}

template <class T>
void wr(uint8_t* p, uint32_t v)
{
    const T t = (T)v;
    std::memcpy(p, &t, sizeof(T));
}

template <class T, int CN>
void apply(const uint8_t* src, int64_t pitch_s, uint8_t* dst, int64_t pitch_d, int h, int w, const Geom& g, const uint16_t* tab, int blocks)
{
    constexpr int ES = sizeof(T), BPP = CN * ES, CC = CN == 1 ? 1 : 3;
    constexpr uint32_t kMax = ES == 1 ? 255u : 65535u;
    const int per_row = segs_of(w) + 1;
    const int64_t items = (int64_t)h * per_row;
    for (int64_t t = 0; t < (int64_t)blocks * kThreads; t++)
        for (int64_t it = t; it < items; it += (int64_t)blocks * kThreads) {
            const int y = (int)(it / per_row), s = (int)(it - (int64_t)y * per_row);
            const uint8_t* rs = src + (int64_t)y * pitch_s;
            uint8_t* rdst = dst + (int64_t)y * pitch_d;
            const int64_t dy2 = sq(y - g.cy);
            const int x0 = head_of((unsigned)((uintptr_t)rdst & 15u), BPP, w);
            const int nseg = (w - x0) / kSegPixels;
            const int x1 = x0 + nseg * kSegPixels;
            if (s < per_row - 1) {
                if (s >= nseg)
                    continue;
                const int xa = x0 + s * kSegPixels;
                uint8_t a[kSegPixels * BPP];  // the segment read whole, then written whole, as the kernel's registers
                std::memcpy(a, rs + (int64_t)xa * BPP, sizeof(a));
                for (int p = 0; p < kSegPixels; p++) {
                    const Pos pos = position(dy2 + sq(xa + p - g.cx), g.scale, g.shift);
                    for (int c = 0; c < CC; c++)
                        wr<T>(a + (p * CN + c) * ES, scaled(rd<T>(a + (p * CN + c) * ES), gain_q14(tab + table_of<CN>(c) * (kBins + 1), pos), kMax));
                }
                std::memcpy(rdst + (int64_t)xa * BPP, a, sizeof(a));
            } else {
                for (int x = 0; x < w; x++) {
                    if (x >= x0 && x < x1)
                        continue;
                    const Pos pos = position(dy2 + sq(x - g.cx), g.scale, g.shift);
                    uint32_t v[CN];
                    for (int c = 0; c < CN; c++)
                        v[c] = rd<T>(rs + ((int64_t)x * CN + c) * ES);
                    for (int c = 0; c < CN; c++)
                        wr<T>(rdst + ((int64_t)x * CN + c) * ES, c < CC ? scaled(v[c], gain_q14(tab + table_of<CN>(c) * (kBins + 1), pos), kMax) : v[c]);
                }
            }
        }
}

struct WaveAdd {
    uint32_t* mine;
    void operator()(int ring, int word, uint32_t value) const { mine[ring * kRingWords + word] += value; }
};

template <class T, int CN>
void rings(const uint8_t* src, int64_t pitch, int h, int w, const RingParams& prm, int blocks, uint64_t* out)
{
    constexpr int ES = sizeof(T), BPP = CN * ES, CC = CN == 1 ? 1 : 3;
    const int words = prm.rings * kRingWords;
    const int per_row = segs_of(w) + 1;
    const int64_t items = (int64_t)h * per_row, stride = (int64_t)blocks * kThreads;
    const int64_t rounds = (items + stride - 1) / stride;
    for (int blk = 0; blk < blocks; blk++) {
        std::vector<uint32_t> copies((size_t)kWaves * words, 0);
        std::vector<RingRun> runs(kThreads);
        for (int64_t r0 = 0; r0 < rounds; r0 += kFlushItems) {
            const int64_t r1 = r0 + kFlushItems < rounds ? r0 + kFlushItems : rounds;
            for (int tid = 0; tid < kThreads; tid++) {
                WaveAdd add{copies.data() + (size_t)(tid >> 6) * words};
                RingRun& run = runs[tid];
                for (int64_t r = r0; r < r1; r++) {
                    const int64_t it = r * stride + (int64_t)blk * kThreads + tid;
                    if (it >= items)
                        continue;
                    const int y = (int)(it / per_row), s = (int)(it - (int64_t)y * per_row);
                    const uint8_t* rs = src + (int64_t)y * pitch;
                    const int64_t dy2 = sq(y - prm.cy);
                    const int x0 = head_of((unsigned)((uintptr_t)rs & 15u), BPP, w);
                    const int nseg = (w - x0) / kSegPixels;
                    const int x1 = x0 + nseg * kSegPixels;
                    int xa = 0, xb = w;  // this item's pixels: a segment, or the head and the tail
                    if (s < per_row - 1) {
                        if (s >= nseg)
                            continue;
                        xa = x0 + s * kSegPixels;
                        xb = xa + kSegPixels;
                    }
                    for (int x = xa; x < xb; x++) {
                        if (s == per_row - 1 && x >= x0 && x < x1)
                            continue;
                        int v[CC];
                        for (int c = 0; c < CC; c++)
                            v[c] = (int)rd<T>(rs + ((int64_t)x * CN + c) * ES);
                        ring_pixel<CC>(v, dy2 + sq(x - prm.cx), prm, run, add);
                    }
                }
                ring_flush(run, add);
            }
            for (int i = 0; i < words; i++) {
                uint64_t t = 0;
                for (int v = 0; v < kWaves; v++) {
                    t += copies[(size_t)v * words + i];
                    copies[(size_t)v * words + i] = 0;
                }
                out[i] += t;
            }
        }
    }
}

}  // namespace

#define VIG_DISPATCH(FN, ...)                              \
    do {                                                   \
        if (es == 1) {                                     \
            if (cn == 1)                                   \
                FN<uint8_t, 1>(__VA_ARGS__);               \
            else if (cn == 3)                              \
                FN<uint8_t, 3>(__VA_ARGS__);               \
            else                                           \
                FN<uint8_t, 4>(__VA_ARGS__);               \
        } else {                                           \
            if (cn == 1)                                   \
                FN<uint16_t, 1>(__VA_ARGS__);              \
            else if (cn == 3)                              \
                FN<uint16_t, 3>(__VA_ARGS__);              \
            else                                           \
                FN<uint16_t, 4>(__VA_ARGS__);              \
        }                                                  \
    } while (0)

// geom: cx, cy, scale, shift (int64 each).  tables: 3 x 1025 uint16.
extern "C" void vignette_emul_apply(const void* src, int64_t pitch_s, void* dst, int64_t pitch_d, int h, int w, int cn, int es,
                                    const int64_t* geom, const uint16_t* tables, int blocks)
{
    const Geom g{(int32_t)geom[0], (int32_t)geom[1], (uint32_t)geom[2], (int32_t)geom[3]};
    VIG_DISPATCH(apply, (const uint8_t*)src, pitch_s, (uint8_t*)dst, pitch_d, h, w, g, tables, blocks);
}

// prm: cx, cy, R2, rings, lo, hi (int64 each).  out: rings x 4 int64, zeroed here.
extern "C" void vignette_emul_rings(const void* src, int64_t pitch, int h, int w, int cn, int es, const int64_t* prm, int blocks, int64_t* out)
{
    const RingParams p{(int32_t)prm[0], (int32_t)prm[1], prm[2], (int32_t)prm[3], (int32_t)prm[4], (int32_t)prm[5]};
    std::memset(out, 0, (size_t)p.rings * kRingWords * sizeof(int64_t));
    VIG_DISPATCH(rings, (const uint8_t*)src, pitch, h, w, p, blocks, (uint64_t*)out);
}

extern "C" int64_t vignette_emul_max_r2(int h, int w, int cx, int cy) { return max_r2(h, w, cx, cy); }

#ifdef VIGNETTE_MAIN
// vignette_san LIST: every line of LIST is "h w cn es offset pitch inplace cx cy scale shift R2 rings lo hi blocks file tables": the
// image is a view into ONE heap copy of the file's exact size, the tables a heap copy of 3 x 1025 uint16.  inplace 1: rewritten where
// it is; 0: into a buffer of exactly h * w * cn * es bytes.  Prints the ring record (taken first) and the result's bytes (hex).
static uint8_t* slurp(const char* path, long* size)
{
    FILE* fp = std::fopen(path, "rb");
    if (!fp)
        return nullptr;
    std::fseek(fp, 0, SEEK_END);
    *size = std::ftell(fp);
    std::fseek(fp, 0, SEEK_SET);
    uint8_t* buf = (uint8_t*)std::malloc(*size > 0 ? *size : 1);
    if (std::fread(buf, 1, *size, fp) != (size_t)*size)
        return nullptr;
    std::fclose(fp);
    return buf;
}

int main(int argc, char** argv)
{
    if (argc != 2)
        return 2;
    FILE* list = std::fopen(argv[1], "r");
    if (!list)
        return 2;
    int h, w, cn, es, inplace, blocks;
    long long off, pitch, geom[4], prm[6];
    char path[4096], tpath[4096];
    while (std::fscanf(list, "%d %d %d %d %lld %lld %d %lld %lld %lld %lld %lld %lld %lld %lld %d %4095s %4095s", &h, &w, &cn, &es, &off, &pitch,
                       &inplace, &geom[0], &geom[1], &geom[2], &geom[3], &prm[2], &prm[3], &prm[4], &prm[5], &blocks, path, tpath) == 18) {
        long size = 0, tsize = 0;
        uint8_t* buf = slurp(path, &size);
        uint8_t* tab = slurp(tpath, &tsize);
        if (!buf || !tab || tsize != (long)(kTableWords * sizeof(uint16_t)))
            return 3;
        const int64_t g64[4] = {geom[0], geom[1], geom[2], geom[3]};
        const int64_t p64[6] = {geom[0], geom[1], prm[2], prm[3], prm[4], prm[5]};
        std::vector<int64_t> rec((size_t)prm[3] * kRingWords);
        vignette_emul_rings(buf + off, pitch, h, w, cn, es, p64, blocks, rec.data());
        const size_t row = (size_t)w * cn * es;
        uint8_t* dst = inplace ? buf + off : (uint8_t*)std::malloc((size_t)h * row);
        const int64_t pd = inplace ? pitch : (int64_t)row;
        vignette_emul_apply(buf + off, pitch, dst, pd, h, w, cn, es, g64, (const uint16_t*)tab, blocks);
        for (size_t i = 0; i < rec.size(); i++)
            std::printf("%lld ", (long long)rec[i]);
        for (int y = 0; y < h; y++)
            for (size_t x = 0; x < row; x++)
                std::printf("%02x", dst[(int64_t)y * pd + x]);
        std::printf("\n");
        if (!inplace)
            std::free(dst);
        std::free(buf);
        std::free(tab);
    }
    std::fclose(list);
    return 0;
}
#endif
