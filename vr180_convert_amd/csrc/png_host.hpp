// png_host.hpp -- host side of the device PNG encoder between its two passes: length-limited Huffman codes from a band's histogram,
// the dynamic block header, the exact size of the coded band, stored or coded, and the words the host asks the device to OR into the
// stream (headers, end-of-block codes, stored-block headers).  Host code only; png.hip and tests/host_png/png_emul.hip include it.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "png_core.hpp"

namespace v1c {
namespace png {

// Optimal length-limited prefix code, with a stated rule so that every implementation gives the same lengths.  The used symbols are
// sorted by (count, symbol).  First the Huffman tree by the two-queue construction (the lighter front of the leaf queue and the
// package queue is taken, the leaf when they weigh the same); if no leaf lies deeper than the limit, its depths are the lengths.
// Otherwise package-merge (Larmore & Hirschberg 1990): on every level the sorted leaves are merged with the
// packages of the level before (pairs of neighbours, a trailing odd item dropped), a leaf going first when the weights are equal;
// the first 2 n - 2 items of the last level are taken and a symbol's length is the number of times its leaf occurs in them.
// Fewer than two used symbols: the used one (symbol 0 if there is none) and the lowest other symbol get one bit each, so that the
// code is complete.  len[i] = 0 for unused symbols.
inline void code_lengths(const uint64_t* freq, int n, int limit, uint8_t* len)
{
    std::fill(len, len + n, (uint8_t)0);
    std::vector<int> used;
    for (int i = 0; i < n; i++)
        if (freq[i])
            used.push_back(i);
    if (used.size() < 2) {
        const int a = used.empty() ? 0 : used[0];
        len[a] = 1;
        len[a == 0 ? 1 : 0] = 1;
        return;
    }
    std::stable_sort(used.begin(), used.end(), [&](int x, int y) { return freq[x] < freq[y]; });
    const int m = (int)used.size();
    {
        // the common case: the Huffman tree itself is within the limit (nodes 0..m-1 are the leaves, m.. the packages in order of making)
        std::vector<uint64_t> w(2 * m - 1);
        std::vector<int> parent(2 * m - 1, -1);
        for (int i = 0; i < m; i++)
            w[i] = freq[used[i]];
        int a = 0, b = m, end = m;
        auto take = [&]() { return (b >= end || (a < m && w[a] <= w[b])) ? a++ : b++; };
        while (end < 2 * m - 1) {
            const int x = take(), y = take();
            w[end] = w[x] + w[y];
            parent[x] = parent[y] = end++;
        }
        std::vector<int> depth(2 * m - 1, 0);
        int deepest = 0;
        for (int i = 2 * m - 3; i >= 0; i--) {
            depth[i] = depth[parent[i]] + 1;
            deepest = std::max(deepest, depth[i]);
        }
        if (deepest <= limit) {
            for (int i = 0; i < m; i++)
                len[used[i]] = (uint8_t)depth[i];
            return;
        }
    }
    // package-merge.  Only weights and leaf / package flags are kept: the packages of a level are pairs of neighbours of the level
    // below IN ORDER, so the first p packages taken on a level are the first 2 p items of the level below, and the leaves taken on
    // a level are a prefix of the sorted leaves; a symbol's length is the number of levels on which its leaf is taken.
    struct Item {
        uint64_t w;
        bool leaf;
    };
    std::vector<std::vector<Item>> lists((size_t)limit);
    for (int level = 0; level < limit; level++) {
        std::vector<Item>& cur = lists[(size_t)level];
        const std::vector<Item>* below = level ? &lists[(size_t)level - 1] : nullptr;
        const size_t npk = below ? below->size() / 2 : 0;
        cur.reserve((size_t)m + npk);
        size_t a = 0, b = 0;
        while (a < (size_t)m || b < npk) {
            const uint64_t pw = b < npk ? (*below)[2 * b].w + (*below)[2 * b + 1].w : 0;
            if (b >= npk || (a < (size_t)m && freq[used[a]] <= pw)) {
                cur.push_back({freq[used[a]], true});
                a++;
            } else {
                cur.push_back({pw, false});
                b++;
            }
        }
    }
    size_t need = 2 * (size_t)m - 2;
    for (int level = limit - 1; level >= 0 && need; level--) {
        const std::vector<Item>& cur = lists[(size_t)level];
        size_t leaves = 0;
        for (size_t i = 0; i < need && i < cur.size(); i++)
            leaves += cur[i].leaf;
        for (size_t k = 0; k < leaves; k++)
            len[used[k]]++;
        need = 2 * (std::min(need, cur.size()) - leaves);
    }
}

// canonical codes (RFC 1951 3.2.2), bit-reversed so that they go out LSB first
inline void canonical_codes(const uint8_t* len, int n, uint32_t* rev)
{
    uint32_t next[kMaxBits + 2] = {0}, count[kMaxBits + 2] = {0};
    for (int i = 0; i < n; i++)
        count[len[i]]++;
    count[0] = 0;
    uint32_t code = 0;
    for (int b = 1; b <= kMaxBits; b++) {
        code = (code + count[b - 1]) << 1;
        next[b] = code;
    }
    for (int i = 0; i < n; i++) {
        rev[i] = 0;
        if (!len[i])
            continue;
        const uint32_t c = next[len[i]]++;
        for (int b = 0; b < len[i]; b++)
            rev[i] |= ((c >> b) & 1u) << (len[i] - 1 - b);
    }
}

struct BitWriter {
    std::vector<uint32_t> words;
    uint64_t nbits = 0;
    void put(uint32_t v, int k)  // k <= 16 bits, LSB first
    {
        if (!k)
            return;
        const size_t wi = (size_t)(nbits >> 5);
        const int sh = (int)(nbits & 31);
        if (words.size() < wi + 2)
            words.resize(wi + 2, 0);
        const uint64_t x = (uint64_t)v << sh;
        words[wi] |= (uint32_t)x;
        words[wi + 1] |= (uint32_t)(x >> 32);
        nbits += k;
    }
};

struct BandPlan {
    bool stored = false;
    uint64_t size = 0;          // bytes of the band's segment of the stream
    uint32_t table[kSymbols];   // (reversed code << 4) | length
    BitWriter header;           // BFINAL = 0, BTYPE = 2, the counts, the code-length code, the lengths
    uint64_t token_bits = 0;    // all tokens without the end-of-block code
    uint32_t eob_rev = 0;
    int eob_len = 0;
};

// hist: the band's literal / length counts from pass 1 (hist[256] is ignored: one end-of-block).  nbytes: its scanline bytes.
inline void plan_band(const uint32_t* hist, uint32_t nbytes, BandPlan& p)
{
    static const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint64_t freq[kSymbols];
    for (int i = 0; i < kSymbols; i++)
        freq[i] = hist[i];
    freq[kEob] = 1;
    uint8_t len[kSymbols];
    code_lengths(freq, kSymbols, kMaxBits, len);
    uint32_t rev[kSymbols];
    canonical_codes(len, kSymbols, rev);
    int hlit = 257;
    for (int i = 257; i < kSymbols; i++)
        if (len[i])
            hlit = i + 1;
    // the lengths as sent: hlit literal / length codes and ONE distance code of one bit; no run-length symbols (16, 17, 18 unused)
    std::vector<uint8_t> sent(len, len + hlit);
    sent.push_back(1);
    uint64_t clf[19] = {0};
    for (uint8_t v : sent)
        clf[v]++;
    uint8_t cl[19];
    code_lengths(clf, 19, 7, cl);
    uint32_t clrev[19];
    canonical_codes(cl, 19, clrev);
    int hclen = 4;
    for (int i = 0; i < 19; i++)
        if (cl[order[i]])
            hclen = std::max(hclen, i + 1);
    p.header = BitWriter();
    p.header.put(0, 1);
    p.header.put(2, 2);
    p.header.put((uint32_t)(hlit - 257), 5);
    p.header.put(0, 5);
    p.header.put((uint32_t)(hclen - 4), 4);
    for (int i = 0; i < hclen; i++)
        p.header.put(cl[order[i]], 3);
    for (uint8_t v : sent)
        p.header.put(clrev[v], cl[v]);
    p.token_bits = 0;
    for (int i = 0; i < kSymbols; i++) {
        p.table[i] = (rev[i] << 4) | len[i];
        if (i == kEob || !hist[i])
            continue;
        int extra = 0;
        if (i >= 265 && i < 285)
            extra = (i - 261) / 4;
        p.token_bits += (uint64_t)hist[i] * (uint64_t)(len[i] + extra + (i > kEob ? 1 : 0));
    }
    p.eob_rev = rev[kEob];
    p.eob_len = len[kEob];
    // header, tokens, end of block, the 3 header bits of an empty stored block, padding to a byte, then 00 00 FF FF
    const uint64_t bits = p.header.nbits + p.token_bits + (uint64_t)p.eob_len + 3;
    const uint64_t coded = (bits + 7) / 8 + 4;
    const uint64_t raw = stored_size(nbytes);
    p.stored = coded > raw;
    p.size = p.stored ? raw : coded;
}

inline void or_bits(std::vector<OrWord>& list, uint64_t bitpos, uint32_t value, int nbits)
{
    if (!nbits || !value)
        return;
    const uint64_t x = (uint64_t)value << (bitpos & 31);
    if ((uint32_t)x)
        list.push_back({bitpos >> 5, (uint32_t)x, 0});
    if ((uint32_t)(x >> 32))
        list.push_back({(bitpos >> 5) + 1, (uint32_t)(x >> 32), 0});
}

// everything of a band that is not a token or a stored data byte, as words to OR into the zeroed stream; `offset`: the band's first byte
inline void band_or_words(const BandPlan& p, uint64_t offset, uint32_t nbytes, std::vector<OrWord>& list)
{
    const uint64_t base = offset * 8;
    if (p.stored) {
        for (uint32_t o = 0; o < nbytes; o += kStoredMax) {
            const uint32_t n = std::min(kStoredMax, nbytes - o);
            const uint64_t at = base + 8 * (stored_position(o) - 5);  // 00, LEN, NLEN (little-endian)
            or_bits(list, at + 8, n, 16);
            or_bits(list, at + 24, n ^ 0xFFFFu, 16);
        }
        return;
    }
    for (uint64_t b = 0; b < p.header.nbits; b += 16)
        or_bits(list, base + b, (p.header.words[(size_t)(b >> 5)] >> (b & 31)) & 0xFFFFu, 16);
    const uint64_t eob = p.header.nbits + p.token_bits;
    or_bits(list, base + eob, p.eob_rev, p.eob_len);
    const uint64_t tail = (eob + (uint64_t)p.eob_len + 3 + 7) / 8;  // the byte after the padding: LEN = 0000, NLEN = FFFF
    or_bits(list, base + 8 * (tail + 2), 0xFFFFu, 16);
}

// ---- the whole image ------------------------------------------------------------------------------------------------------------

struct Layout {
    int bpp = 0;                 // bytes per pixel
    uint32_t h = 0, stride = 0;  // rows; scanline bytes with the filter byte
    uint32_t band_rows = 0, n_bands = 0;
    uint32_t segs_per_band = 0, groups = 0;
    uint32_t band_bytes(uint32_t band) const { return std::min(band_rows, h - band * band_rows) * stride; }
};

// false for arguments outside the contract (include/vr180_remap.h, v1c_png_deflate)
inline bool make_layout(int h, int w, int cn, int depth, int band_rows, Layout& l)
{
    const int nb = depth == 0 ? 1 : depth == 2 ? 2 : 0;  // V1C_DEPTH_8U / V1C_DEPTH_16U
    if (!nb || (cn != 1 && cn != 3 && cn != 4) || h < 1 || w < 1 || h > (1 << 20) || w > (1 << 20) || band_rows < 1)
        return false;
    l.bpp = cn * nb;
    l.h = (uint32_t)h;
    l.stride = 1u + (uint32_t)w * (uint32_t)l.bpp;
    l.band_rows = (uint32_t)std::min(band_rows, h);
    if ((uint64_t)l.band_rows * l.stride > 0x7fffffffull)
        return false;
    l.n_bands = (l.h + l.band_rows - 1) / l.band_rows;
    l.segs_per_band = (l.band_rows * l.stride + kSeg - 1) / kSeg;
    l.groups = (l.segs_per_band + kSegsPerGroup - 1) / kSegsPerGroup;
    return (uint64_t)l.n_bands * l.groups < 0x7fffffffull;
}

inline uint64_t bound(const Layout& l)
{
    uint64_t n = 0;
    for (uint32_t b = 0; b < l.n_bands; b++)
        n += stored_size(l.band_bytes(b)) + 8;
    return n;
}

struct Plan {
    std::vector<BandPlan> bands;
    std::vector<uint64_t> offset;   // of every band's segment of the stream
    std::vector<BandDev> dev;
    std::vector<uint32_t> tables;   // n_bands x kSymbols
    std::vector<OrWord> ors;
    uint64_t total = 0;
    bool any_coded = false, any_stored = false;
};

// everything the host decides between the passes, from the n_bands x kHistStride counts of pass 1
inline void plan_image(const Layout& l, const uint32_t* hist, Plan& p)
{
    p.bands.resize(l.n_bands);
    p.offset.resize(l.n_bands);
    p.dev.resize(l.n_bands);
    p.tables.resize((size_t)l.n_bands * kSymbols);
    p.ors.clear();
    p.total = 0;
    p.any_coded = p.any_stored = false;
    for (uint32_t b = 0; b < l.n_bands; b++) {
        BandPlan& bp = p.bands[b];
        plan_band(hist + (size_t)b * kHistStride, l.band_bytes(b), bp);
        p.offset[b] = p.total;
        p.dev[b] = BandDev{8 * p.total + bp.header.nbits, p.total, bp.stored ? 1u : 0u, 0u};
        std::copy(bp.table, bp.table + kSymbols, p.tables.begin() + (size_t)b * kSymbols);
        band_or_words(bp, p.total, l.band_bytes(b), p.ors);
        (bp.stored ? p.any_stored : p.any_coded) = true;
        p.total += bp.size;
    }
}

// Adler-32 of a band from pass 1's sums: a = sum of its n bytes, b = sum of (n - i) * byte[i] (any representative modulo 65521)
inline uint32_t band_adler(uint64_t a, uint64_t b, uint32_t n)
{
    const uint64_t s1 = (1 + a) % kAdlerBase, s2 = (n + b) % kAdlerBase;
    return (uint32_t)(s1 | (s2 << 16));
}

}  // namespace png
}  // namespace v1c
