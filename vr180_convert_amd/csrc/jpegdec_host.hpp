// jpegdec_host.hpp -- host side of the device JPEG decoder: the marker parser, the construction of the decoder's tables, the geometry
// and the walk over the scan's 0xFF bytes that finds the scan's end and its RSTm markers.  Everything a file can be refused for without
// decoding it is found here, before the device is touched (v1c_jpeg_decode_info is this parse alone), and the rule of subseq_bits of
// every entry that decodes (subseq_of).  Shared by jpegdec.hip, the lossless entries (jpegx_chain.hpp) and the
// host harness (tests/host_jpegdec/jpegdec_emul.hip); tests/jpgdec_ref.py restates it.
#pragma once

#include <cstring>
#include <string>
#include <vector>

#include "jpegdec_core.hpp"

namespace v1c {
namespace jpegdec {

enum ParseResult { kParsed = 0, kUnsupported = 1, kCorrupt = 2 };

struct Parsed {
    Geom g;
    Tables tab;
    uint32_t restart = 0;                // DRI's value
    uint64_t scan_start = 0, scan_len = 0;  // the stuffed scan in the file, up to the marker that ends it
    std::vector<uint32_t> segoff;        // nseg + 1: bytes of the unstuffed stream where every segment begins
    uint64_t error_pos = 0;              // byte of the file
    std::string why;
};

// (bits, vals) of a DHT table to the decoder's form; false where a length holds more codes than it can
inline bool make_table(const uint8_t* bits, const uint8_t* vals, int count, Table& t)
{
    std::memset(&t, 0, sizeof(t));
    std::memcpy(t.vals, vals, (size_t)count);
    int32_t code = 0, k = 0;
    for (int n = 1; n <= 16; n++) {
        t.valoff[n] = k - code;
        if (code + bits[n - 1] > 1 << n)  // (before anything is filled: the lookup has room for the codes a length can hold, no more)
            return false;
        for (int i = 0; i < bits[n - 1]; i++, code++, k++)
            if (n <= kLutBits)
                for (int j = 0; j < 1 << (kLutBits - n); j++)
                    t.lut[(code << (kLutBits - n)) + j] = (uint16_t)(n << 8 | vals[k]);
        t.maxcode[n] = bits[n - 1] ? code - 1 : -1;
        code <<= 1;
    }
    t.maxcode[17] = -1;
    return true;
}

namespace detail {

inline ParseResult fail(Parsed& out, ParseResult r, uint64_t pos, const char* why)
{
    out.error_pos = pos, out.why = why;
    return r;
}

inline uint32_t be16(const uint8_t* d)
{
    return (uint32_t)d[0] << 8 | d[1];
}

}  // namespace detail

inline ParseResult parse(const uint8_t* d, uint64_t n, Parsed& out)
{
    using detail::be16;
    using detail::fail;
    if (n < 4 || d[0] != 0xff || d[1] != 0xd8)
        return fail(out, kCorrupt, 0, "no SOI");
    Geom& g = out.g;
    std::memset(&g, 0, sizeof(g));
    bool have_q[4] = {}, have_dc[4] = {}, have_ac[4] = {}, have_frame = false;
    uint8_t comp_id[3] = {}, comp_h[3] = {}, comp_v[3] = {}, comp_q[3] = {};
    int adobe = -1;
    uint64_t pos = 2;
    for (;;) {
        if (pos + 1 >= n || d[pos] != 0xff)
            return fail(out, kCorrupt, pos, "marker expected");
        while (pos + 1 < n && d[pos + 1] == 0xff)
            pos++;  // fill bytes
        if (pos + 1 >= n)
            return fail(out, kCorrupt, pos, "the file ends in a marker");
        const uint8_t m = d[pos + 1];
        pos += 2;
        if (m == 0x01 || (m >= 0xd0 && m <= 0xd7))
            continue;
        if (m == 0xd8 || m == 0xd9)
            return fail(out, kCorrupt, pos - 2, "SOI or EOI before the scan");
        if (pos + 2 > n)
            return fail(out, kCorrupt, pos, "segment length");
        const uint32_t ln = be16(d + pos);
        if (ln < 2 || pos + ln > n)
            return fail(out, kCorrupt, pos, "segment length");
        const uint8_t* body = d + pos + 2;
        const uint32_t nb = ln - 2;
        if (m == 0xc0 || m == 0xc1) {
            if (have_frame || nb < 6 || nb != 6u + 3u * body[5])
                return fail(out, kCorrupt, pos, "SOF");
            if (body[0] != 8)
                return fail(out, kUnsupported, pos, "samples of other than 8 bits");
            g.h = be16(body + 1), g.w = be16(body + 3), g.nc = body[5];
            if (g.h == 0)
                return fail(out, kUnsupported, pos, "height 0: DNL");
            if (g.w == 0)
                return fail(out, kCorrupt, pos, "width 0");
            if (g.nc != 1 && g.nc != 3)
                return fail(out, kUnsupported, pos, "neither one component nor three");
            for (uint32_t i = 0; i < g.nc; i++)
                comp_id[i] = body[6 + 3 * i], comp_h[i] = body[7 + 3 * i] >> 4, comp_v[i] = body[7 + 3 * i] & 15, comp_q[i] = body[8 + 3 * i];
            have_frame = true;
        } else if ((m >= 0xc2 && m <= 0xcf) && m != 0xc4 && m != 0xcc) {
            return fail(out, kUnsupported, pos, "progressive, lossless or arithmetic");
        } else if (m == 0xcc) {
            return fail(out, kUnsupported, pos, "arithmetic conditioning");
        } else if (m == 0xc4) {
            for (uint32_t i = 0; i < nb;) {
                if (i + 17 > nb || (body[i] >> 4) > 1 || (body[i] & 15) > 3)
                    return fail(out, kCorrupt, pos, "DHT");
                int cnt = 0;
                for (int k = 0; k < 16; k++)
                    cnt += body[i + 1 + k];
                if (cnt > 256 || i + 17 + cnt > nb)
                    return fail(out, kCorrupt, pos, "DHT");
                const bool ac = body[i] >> 4;
                const int th = body[i] & 15;
                if (!ac)
                    for (int k = 0; k < cnt; k++)
                        if (body[i + 17 + k] > 15)
                            return fail(out, kCorrupt, pos, "DHT: DC category above 15");
                if (!make_table(body + i + 1, body + i + 17, cnt, ac ? out.tab.ac[th] : out.tab.dc[th]))
                    return fail(out, kCorrupt, pos, "DHT: more codes than the length holds");
                (ac ? have_ac : have_dc)[th] = true;
                i += 17 + cnt;
            }
        } else if (m == 0xdb) {
            for (uint32_t i = 0; i < nb;) {
                const uint32_t pq = body[i] >> 4, tq = body[i] & 15;
                if (pq > 1 || tq > 3 || i + 1 + 64 * (pq + 1) > nb)
                    return fail(out, kCorrupt, pos, "DQT");
                for (int nat = 0; nat < 64; nat++) {
                    const int k = zigzag_of(nat);
                    out.tab.q[tq][nat] = (uint16_t)(pq ? be16(body + i + 1 + 2 * k) : body[i + 1 + k]);
                }
                have_q[tq] = true;
                i += 1 + 64 * (pq + 1);
            }
        } else if (m == 0xdd) {
            if (ln != 4)
                return fail(out, kCorrupt, pos, "DRI");
            out.restart = be16(body);
        } else if (m == 0xdc) {
            return fail(out, kUnsupported, pos, "DNL");
        } else if (m == 0xee && nb >= 12 && std::memcmp(body, "Adobe", 5) == 0) {
            adobe = body[11];
        } else if (m == 0xda) {
            if (!have_frame || nb < 1 || nb != 4u + 2u * body[0])
                return fail(out, kCorrupt, pos, "SOS");
            if (body[0] != g.nc)
                return fail(out, kUnsupported, pos, "several scans");
            for (uint32_t i = 0; i < g.nc; i++) {
                if (body[1 + 2 * i] != comp_id[i])
                    return fail(out, kUnsupported, pos, "scan components out of order");
                const uint32_t td = body[2 + 2 * i] >> 4, ta = body[2 + 2 * i] & 15;
                if (td > 3 || ta > 3 || !have_dc[td] || !have_ac[ta] || comp_q[i] > 3 || !have_q[comp_q[i]])
                    return fail(out, kCorrupt, pos, "a table the scan names is missing");
                g.td[i] = (uint8_t)td, g.ta[i] = (uint8_t)ta, g.tq[i] = comp_q[i];
            }
            if (body[nb - 3] != 0 || body[nb - 2] != 63 || body[nb - 1] != 0)
                return fail(out, kUnsupported, pos, "spectral selection or successive approximation");
            pos += ln;
            break;
        }
        pos += ln;
    }
    if (g.nc == 3 && adobe == 0)
        return fail(out, kUnsupported, pos, "Adobe transform 0: RGB");
    if (g.nc == 1) {
        g.hs = g.vs = 1;  // (one component: not interleaved, whatever its factors)
    } else {
        const bool luma = (comp_h[0] == 1 && comp_v[0] == 1) || (comp_h[0] == 2 && comp_v[0] == 1) || (comp_h[0] == 2 && comp_v[0] == 2);
        if (!luma || comp_h[1] != 1 || comp_v[1] != 1 || comp_h[2] != 1 || comp_v[2] != 1)
            return fail(out, kUnsupported, pos, "sampling factors other than 4:4:4, 4:2:2 and 4:2:0");
        g.hs = comp_h[0], g.vs = comp_v[0];
    }
    finish_geom(g);
    g.interval = out.restart ? out.restart : g.nmcu;
    g.nseg = (g.nmcu + g.interval - 1) / g.interval;
    g.ibl = g.interval * g.bpm;
    // the walk over the scan's 0xFF bytes: stuffed zeros, fill bytes and RSTm are dropped (jpegdec_core.hpp: dropped); any other marker
    // ends the scan
    out.scan_start = pos;
    out.segoff.assign(1, 0u);
    uint64_t removed = 0, i = pos, j;
    uint8_t nx;
    for (;;) {
        const void* f = i < n ? std::memchr(d + i, 0xff, n - i) : nullptr;
        if (!f || (uint64_t)((const uint8_t*)f - d) + 1 >= n)
            return fail(out, kCorrupt, n, "no EOI");
        j = (uint64_t)((const uint8_t*)f - d);
        nx = d[j + 1];
        if (nx == 0) {
            removed++, i = j + 2;
        } else if (nx == 0xff) {
            removed++, i = j + 1;
        } else if (nx >= 0xd0 && nx <= 0xd7) {
            const uint64_t k = out.segoff.size() - 1;
            if (out.restart == 0 || (uint32_t)(nx - 0xd0) != (k & 7) || k + 1 >= g.nseg)
                return fail(out, kCorrupt, j, "a restart marker out of sequence");
            out.segoff.push_back((uint32_t)(j - pos - removed));
            removed += 2, i = j + 2;
        } else {
            break;
        }
    }
    if (nx == 0xdc)
        return fail(out, kUnsupported, j, "DNL");
    if (nx != 0xd9)
        return fail(out, kUnsupported, j, "several scans");
    if (out.segoff.size() != g.nseg)
        return fail(out, kCorrupt, j, "restart markers missing");
    out.scan_len = j - pos;
    if (out.scan_len >= (1ull << 32) - 2 * kPiece)
        return fail(out, kUnsupported, pos, "a stuffed scan of 2^32 bytes");
    if ((out.scan_len - removed) * 8 >= (1ull << 31))
        return fail(out, kUnsupported, pos, "a scan of 2^31 bits");
    out.segoff.push_back((uint32_t)(out.scan_len - removed));
    for (size_t k = 0; k + 1 < out.segoff.size(); k++)
        if (out.segoff[k + 1] <= out.segoff[k])
            return fail(out, kCorrupt, pos, "an empty segment");
    return kParsed;
}

// The bits of a subsequence that an entry's subseq_bits asks for, or 0 where it breaks the rule.
inline uint32_t subseq_of(uint32_t subseq_bits)
{
    const uint32_t S = subseq_bits ? subseq_bits : kDefaultSubseqBits;
    return S % 32 || S < 256 || S > (1u << 24) ? 0 : S;
}
constexpr const char* kSubseqRule = "subseq_bits must be a multiple of 32 from 256 to 2^24, or 0";

// the first subsequence of every segment (nseg + 1 entries): a segment's bits are tiled by S, and no subsequence spans two segments
inline std::vector<uint32_t> sub_first(const Parsed& p, uint32_t S)
{
    std::vector<uint32_t> f(p.segoff.size());
    uint64_t at = 0;
    for (size_t k = 0; k + 1 < p.segoff.size(); k++) {
        f[k] = (uint32_t)at;
        at += ((uint64_t)(p.segoff[k + 1] - p.segoff[k]) * 8 + S - 1) / S;
    }
    f.back() = (uint32_t)at;
    return f;
}

inline TablePair table_pair(const Geom& g, const Table* dcs, const Table* acs)
{
    TablePair tp{dcs, acs, 0, 0};
    for (uint32_t c = 0; c < g.bpm; c++) {
        tp.dcsel |= (uint32_t)g.td[comp_of(g, c)] << (4 * c);
        tp.acsel |= (uint32_t)g.ta[comp_of(g, c)] << (4 * c);
    }
    return tp;
}

}  // namespace jpegdec
}  // namespace v1c
