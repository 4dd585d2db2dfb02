// Host access to the compact entry of the pair mirror kernel's tap table (csrc/tap_table.hpp: TapEntry8) for
// tests/test_tap_table_compact_host.py: the product's own tap8_fits / tap8_encode / tap8_decode next to the 12-byte entry's functions,
// compiled for the host.  With -DTAP8_MAIN the same file is a stand-alone program (its own main) that walks the field extremes and a
// fixed pseudo-random sequence -- what the test builds with -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../vr180_convert_amd/csrc/tap_table.hpp"

using namespace v1c;

static TapCoords coords_of(const int* v)
{
    TapCoords c;
    for (int k = 0; k < kTapPX; k++)
        c.x[k] = v[k], c.y[k] = v[4 + k], c.y2[k] = v[8 + k];
    return c;
}

static void coords_to(const TapCoords& d, int* out)
{
    for (int k = 0; k < kTapPX; k++)
        out[k] = d.x[k], out[4 + k] = d.y[k], out[8 + k] = d.y2[k];
}

extern "C" {

int tap8_sizeof()
{
    return (int)sizeof(TapEntry8);
}

// limits[0..8] = base max, dx1 max, dy1 min, dy1 max, second difference min, max, e min, max, pixels per lane
void tap8_limits(int* out)
{
    out[0] = kTapBaseMax, out[1] = kTap8DxMax, out[2] = kTap8DyMin, out[3] = kTap8DyMax, out[4] = kTap8DdMin, out[5] = kTap8DdMax,
    out[6] = kTap8EMin, out[7] = kTap8EMax, out[8] = kTapPX;
}

// n entries of 12 ints (x[4], y[4], y2[4]) with their K: fits -> fit[n], packed words -> words[2 n], decoded again -> back[12 n];
// the 12-byte entry on the same coordinates: fits -> fit12[n], decoded again -> back12[12 n]
void tap8_many(const int* coords, const int* K, int64_t n, uint8_t* fit, uint32_t* words, int* back, uint8_t* fit12, int* back12)
{
    for (int64_t i = 0; i < n; i++) {
        const TapCoords c = coords_of(coords + 12 * i);
        fit[i] = tap8_fits(c, K[i]) ? 1 : 0;
        const TapEntry8 e = tap8_encode(c, K[i]);
        std::memcpy(words + 2 * i, e.w, sizeof(e.w));
        coords_to(tap8_decode(e, K[i]), back + 12 * i);
        fit12[i] = tap_entry_fits(c) ? 1 : 0;
        coords_to(tap_entry_decode(tap_entry_encode(c)), back12 + 12 * i);
    }
}

void tap8_decode_words(const uint32_t* words, int K, int* back)
{
    TapEntry8 e;
    std::memcpy(e.w, words, sizeof(e.w));
    coords_to(tap8_decode(e, K), back);
}
}

#ifdef TAP8_MAIN
static bool same(const TapCoords& a, const TapCoords& b)
{
    return std::memcmp(&a, &b, sizeof(a)) == 0;
}

// coordinates from the entry's own fields
static TapCoords build(int x0, int dx1, const int (&ddx)[2], int y0, int dy1, const int (&ddy)[2], const int (&e)[4], int K)
{
    TapCoords c;
    int dx = dx1, dy = dy1;
    c.x[0] = x0, c.y[0] = y0;
    for (int k = 1; k < kTapPX; k++) {
        if (k > 1)
            dx += ddx[k - 2], dy += ddy[k - 2];
        c.x[k] = c.x[k - 1] + dx, c.y[k] = c.y[k - 1] + dy;
    }
    for (int k = 0; k < kTapPX; k++)
        c.y2[k] = K - c.y[k] + e[k];
    return c;
}

int main()
{
    long bad = 0, n = 0;
    const int bases[] = {0, 1, 31, 32, 2047, kTapBaseMax - 1, kTapBaseMax};
    const int dxs[] = {0, 1, 32, 127, 128, kTap8DxMax};
    const int dys[] = {kTap8DyMin, -33, -32, -1, 0, 1, 31, 32, kTap8DyMax};
    const int dds[] = {kTap8DdMin, -1, 0, kTap8DdMax};
    const int es[] = {kTap8EMin, -1, 0, kTap8EMax};
    const int Ks[] = {-70000, 0, 4711, 262144};
    for (int b : bases)
        for (int dx : dxs)
            for (int dy : dys)
                for (int dd : dds)
                    for (int e : es)
                        for (int K : Ks) {
                            const int ddx[2] = {dd, -1 - dd}, ddy[2] = {-1 - dd, dd}, ev[4] = {e, -1 - e, e, kTap8EMax};
                            const TapCoords c = build(b, dx, ddx, b, dy, ddy, ev, K);
                            bad += !tap8_fits(c, K) || !same(tap8_decode(tap8_encode(c, K), K), c);
                            n++;
                        }
    uint32_t s = 12345u;
    auto rnd = [&](uint32_t m) { return (int)((s = s * 1664525u + 1013904223u) >> 8) % (int)m; };
    auto in = [&](int lo, int hi) { return lo + rnd((uint32_t)(hi - lo + 1)); };
    for (int i = 0; i < 200000; i++) {
        const int ddx[2] = {in(kTap8DdMin, kTap8DdMax), in(kTap8DdMin, kTap8DdMax)}, ddy[2] = {in(kTap8DdMin, kTap8DdMax), in(kTap8DdMin, kTap8DdMax)};
        const int ev[4] = {in(kTap8EMin, kTap8EMax), in(kTap8EMin, kTap8EMax), in(kTap8EMin, kTap8EMax), in(kTap8EMin, kTap8EMax)};
        const int K = in(-100000, 400000);
        const TapCoords c = build(in(0, kTapBaseMax), in(0, kTap8DxMax), ddx, in(0, kTapBaseMax), in(kTap8DyMin, kTap8DyMax), ddy, ev, K);
        bad += !tap8_fits(c, K) || !same(tap8_decode(tap8_encode(c, K), K), c);
        n++;
    }
    // one step outside a range: not fitting, and encoding it anyway stays inside the entry
    const int z2[2] = {0, 0}, z4[4] = {0, 0, 0, 0};
    {
        const TapCoords c = build(kTapBaseMax + 1, 0, z2, 0, 0, z2, z4, 100);
        bad += tap8_fits(c, 100);
        (void)tap8_encode(c, 100);
    }
    {
        const TapCoords c = build(0, -1, z2, 0, 0, z2, z4, 100);
        bad += tap8_fits(c, 100);
        (void)tap8_encode(c, 100);
    }
    {
        const int d[2] = {kTap8DdMax + 1, 0};
        const TapCoords c = build(0, 5, z2, 100, 0, d, z4, 100);
        bad += tap8_fits(c, 100);
        (void)tap8_encode(c, 100);
    }
    {
        const int e[4] = {0, 0, kTap8EMin - 1, 0};
        const TapCoords c = build(0, 5, z2, 100, 0, z2, e, 100);
        bad += tap8_fits(c, 100);
        (void)tap8_encode(c, 100);
    }
    {  // far outside: the differences stay inside int
        TapCoords c{};
        c.x[1] = 1 << 28, c.y[2] = -(1 << 28), c.y2[3] = 1 << 28;
        bad += tap8_fits(c, 1 << 20);
        (void)tap8_encode(c, 1 << 20);
    }
    std::printf("compact tap table entries: %ld checked, %ld bad\n", n, bad);
    return bad ? 1 : 0;
}
#endif
