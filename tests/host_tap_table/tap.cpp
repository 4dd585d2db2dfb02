// Host access to the pair mirror kernel's tap-table entry (csrc/tap_table.hpp) for tests/test_tap_table_host.py: the product's own
// encode / decode / fits functions, compiled for the host.  With -DTAP_MAIN the same file is a stand-alone program (its own main)
// that walks the field extremes and a fixed pseudo-random sequence -- what the test builds with -fsanitize=address,undefined.
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

extern "C" {

int tap_sizeof()
{
    return (int)sizeof(TapEntry);
}

// limits[0..4] = base max, dx max, dy min, dy max, pixels per lane
void tap_limits(int* out)
{
    out[0] = kTapBaseMax, out[1] = kTapDxMax, out[2] = kTapDyMin, out[3] = kTapDyMax, out[4] = kTapPX;
}

// n entries of 12 ints (x[4], y[4], y2[4]): fits -> fit[n], packed words -> words[3 n], decoded again -> back[12 n]
void tap_many(const int* coords, int64_t n, uint8_t* fit, uint32_t* words, int* back)
{
    for (int64_t i = 0; i < n; i++) {
        const TapCoords c = coords_of(coords + 12 * i);
        fit[i] = tap_entry_fits(c) ? 1 : 0;
        const TapEntry e = tap_entry_encode(c);
        std::memcpy(words + 3 * i, e.w, sizeof(e.w));
        const TapCoords d = tap_entry_decode(e);
        for (int k = 0; k < kTapPX; k++)
            back[12 * i + k] = d.x[k], back[12 * i + 4 + k] = d.y[k], back[12 * i + 8 + k] = d.y2[k];
    }
}

void tap_decode(const uint32_t* words, int* back)
{
    TapEntry e;
    std::memcpy(e.w, words, sizeof(e.w));
    const TapCoords d = tap_entry_decode(e);
    for (int k = 0; k < kTapPX; k++)
        back[k] = d.x[k], back[4 + k] = d.y[k], back[8 + k] = d.y2[k];
}
}

#ifdef TAP_MAIN
static bool same(const TapCoords& a, const TapCoords& b)
{
    return std::memcmp(&a, &b, sizeof(a)) == 0;
}

int main()
{
    long bad = 0, n = 0;
    const int bases[] = {0, 1, 31, 32, 2047, kTapBaseMax - 1, kTapBaseMax};
    const int dxs[] = {0, 1, 32, 63, 64, kTapDxMax};
    const int dys[] = {kTapDyMin, -13, -1, 0, 1, 13, kTapDyMax};
    for (int b : bases)
        for (int dx : dxs)
            for (int dy : dys)
                for (int dy2 : dys) {
                    TapCoords c;
                    // (the y bases leave room for three steps either way)
                    const int yb = b < 96 ? 96 : (b > kTapBaseMax - 96 ? kTapBaseMax - 96 : b);
                    for (int k = 0; k < kTapPX; k++)
                        c.x[k] = b + k * dx, c.y[k] = yb + k * dy, c.y2[k] = yb + k * dy2;
                    bad += !tap_entry_fits(c) || !same(tap_entry_decode(tap_entry_encode(c)), c);
                    n++;
                }
    uint32_t s = 12345u;
    auto rnd = [&](uint32_t m) { return (int)((s = s * 1664525u + 1013904223u) >> 8) % (int)m; };
    for (int i = 0; i < 200000; i++) {
        TapCoords c;
        c.x[0] = rnd(kTapBaseMax + 1), c.y[0] = rnd(kTapBaseMax + 1), c.y2[0] = rnd(kTapBaseMax + 1);
        for (int k = 1; k < kTapPX; k++) {
            c.x[k] = c.x[k - 1] + rnd(kTapDxMax + 1);
            c.y[k] = c.y[k - 1] + kTapDyMin + rnd(kTapDyMax - kTapDyMin + 1);
            c.y2[k] = c.y2[k - 1] + kTapDyMin + rnd(kTapDyMax - kTapDyMin + 1);
        }
        bad += !tap_entry_fits(c) || !same(tap_entry_decode(tap_entry_encode(c)), c);
        n++;
    }
    // one step outside each range: not fitting, and encoding it anyway stays inside the entry
    TapCoords c{};
    c.x[0] = kTapBaseMax + 1;
    bad += tap_entry_fits(c);
    (void)tap_entry_encode(c);
    c = TapCoords{};
    c.x[1] = -1;
    bad += tap_entry_fits(c);
    (void)tap_entry_encode(c);
    c = TapCoords{};
    c.y[0] = 100, c.y[1] = 100 + kTapDyMax + 1, c.y[2] = c.y[3] = c.y[1];
    bad += tap_entry_fits(c);
    (void)tap_entry_encode(c);
    std::printf("tap table entries: %ld checked, %ld bad\n", n, bad);
    return bad ? 1 : 0;
}
#endif
