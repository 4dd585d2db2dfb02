// jpegprog_host.hpp -- host side of the device decoder of progressive JPEG files: the marker parse over ALL the file's scans.  Per
// scan it keeps the header, the Huffman tables and the restart interval in force, and does jpegdec_host.hpp's memchr walk over the
// entropy-coded bytes: stuffed zeros, fill bytes and RSTm are dropped, any other marker -- a following SOS, DHT, DQT, DRI, or EOI --
// ends the scan.  It follows every coefficient's successive-approximation state through the script, so an illegal script is
// V1C_E_CORRUPT and a script that leaves a coefficient unfinished V1C_E_UNSUPPORTED here, before the device is touched
// (v1c_jpeg_prog_info is this parse alone).  Shared by jpegdec.hip and the host harness (tests/host_jpegdec_prog/jpegprog_emul.hip);
// tests/jpgprog_ref.py restates it.  The marker segments in front of and between the scans are read as jpegdec_host.hpp's parse reads
// them, which is left as it is: it refuses these files at their SOF marker.
#pragma once

#include <cstring>
#include <string>
#include <vector>

#include "jpegdec_host.hpp"
#include "jpegprog_core.hpp"

namespace v1c {
namespace jpegprog {

using jpegdec::kCorrupt;
using jpegdec::kParsed;
using jpegdec::kUnsupported;
using jpegdec::ParseResult;

struct PScan {
    Scan sc;
    uint32_t restart = 0;
    Tables tab;                           // the Huffman tables in force (q: unused)
    uint64_t scan_start = 0, scan_len = 0;  // the stuffed scan in the file, up to the marker that ends it
    std::vector<uint32_t> segoff;         // nseg + 1: bytes of the unstuffed scan where every segment begins
};

struct PParsed {
    Geom g;                               // the frame's; one segment (the pixel stage restarts nowhere); tq[c] = c
    Tables tab;                           // q[c]: component c's table as it stood at the component's first scan (libjpeg latches it there)
    std::vector<PScan> scans;
    uint64_t error_pos = 0;
    std::string why;
};

inline ParseResult parse(const uint8_t* d, uint64_t n, PParsed& out)
{
    using jpegdec::detail::be16;
    auto fail = [&out](ParseResult r, uint64_t pos, const char* why) {
        out.error_pos = pos, out.why = why;
        return r;
    };
    if (n < 4 || d[0] != 0xff || d[1] != 0xd8)
        return fail(kCorrupt, 0, "no SOI");
    Geom& g = out.g;
    std::memset(&g, 0, sizeof(g));
    std::memset(&out.tab, 0, sizeof(out.tab));
    out.scans.clear();
    Tables cur;  // the tables in force
    std::memset(&cur, 0, sizeof(cur));
    bool have_q[4] = {}, have_dc[4] = {}, have_ac[4] = {}, have_frame = false, latched[3] = {};
    uint8_t comp_id[3] = {}, comp_h[3] = {}, comp_v[3] = {}, comp_q[3] = {};
    int8_t bits[3][64];  // the Al every coefficient stands at; -1: no scan yet
    std::memset(bits, -1, sizeof(bits));
    int adobe = -1;
    uint32_t restart = 0;
    uint64_t pos = 2;
    for (;;) {
        if (pos + 1 >= n || d[pos] != 0xff)
            return fail(kCorrupt, pos, "marker expected");
        while (pos + 1 < n && d[pos + 1] == 0xff)
            pos++;  // fill bytes
        if (pos + 1 >= n)
            return fail(kCorrupt, pos, "the file ends in a marker");
        const uint8_t m = d[pos + 1];
        pos += 2;
        if (m == 0x01 || (m >= 0xd0 && m <= 0xd7))
            continue;
        if (m == 0xd9) {
            if (out.scans.empty())
                return fail(kCorrupt, pos - 2, "SOI or EOI before the scan");
            break;
        }
        if (m == 0xd8)
            return fail(kCorrupt, pos - 2, "SOI or EOI before the scan");
        if (pos + 2 > n)
            return fail(kCorrupt, pos, "segment length");
        const uint32_t ln = be16(d + pos);
        if (ln < 2 || pos + ln > n)
            return fail(kCorrupt, pos, "segment length");
        const uint8_t* body = d + pos + 2;
        const uint32_t nb = ln - 2;
        if (m == 0xc2) {
            if (have_frame || nb < 6 || nb != 6u + 3u * body[5])
                return fail(kCorrupt, pos, "SOF");
            if (body[0] != 8)
                return fail(kUnsupported, pos, "samples of other than 8 bits");
            g.h = be16(body + 1), g.w = be16(body + 3), g.nc = body[5];
            if (g.h == 0)
                return fail(kUnsupported, pos, "height 0: DNL");
            if (g.w == 0)
                return fail(kCorrupt, pos, "width 0");
            if (g.nc != 1 && g.nc != 3)
                return fail(kUnsupported, pos, "neither one component nor three");
            for (uint32_t i = 0; i < g.nc; i++)
                comp_id[i] = body[6 + 3 * i], comp_h[i] = body[7 + 3 * i] >> 4, comp_v[i] = body[7 + 3 * i] & 15, comp_q[i] = body[8 + 3 * i];
            if (g.nc == 1) {
                g.hs = g.vs = 1;  // (one component: not interleaved, whatever its factors)
            } else {
                const bool luma = (comp_h[0] == 1 && comp_v[0] == 1) || (comp_h[0] == 2 && comp_v[0] == 1) || (comp_h[0] == 2 && comp_v[0] == 2);
                if (!luma || comp_h[1] != 1 || comp_v[1] != 1 || comp_h[2] != 1 || comp_v[2] != 1)
                    return fail(kUnsupported, pos, "sampling factors other than 4:4:4, 4:2:2 and 4:2:0");
                g.hs = comp_h[0], g.vs = comp_v[0];
            }
            jpegdec::finish_geom(g);
            g.interval = g.nmcu, g.nseg = 1, g.ibl = g.nblocks;
            for (uint32_t i = 0; i < g.nc; i++)
                g.tq[i] = (uint8_t)i;
            have_frame = true;
        } else if (m == 0xc0 || m == 0xc1) {
            return fail(kUnsupported, pos, "a sequential file: v1c_jpeg_decode takes it");
        } else if ((m >= 0xc3 && m <= 0xcf) && m != 0xc4 && m != 0xcc) {
            return fail(kUnsupported, pos, "lossless or arithmetic");
        } else if (m == 0xcc) {
            return fail(kUnsupported, pos, "arithmetic conditioning");
        } else if (m == 0xc4) {
            for (uint32_t i = 0; i < nb;) {
                if (i + 17 > nb || (body[i] >> 4) > 1 || (body[i] & 15) > 3)
                    return fail(kCorrupt, pos, "DHT");
                int cnt = 0;
                for (int k = 0; k < 16; k++)
                    cnt += body[i + 1 + k];
                if (cnt > 256 || i + 17 + cnt > nb)
                    return fail(kCorrupt, pos, "DHT");
                const bool ac = body[i] >> 4;
                const int th = body[i] & 15;
                if (!ac)
                    for (int k = 0; k < cnt; k++)
                        if (body[i + 17 + k] > 15)
                            return fail(kCorrupt, pos, "DHT: DC category above 15");
                if (!jpegdec::make_table(body + i + 1, body + i + 17, cnt, ac ? cur.ac[th] : cur.dc[th]))
                    return fail(kCorrupt, pos, "DHT: more codes than the length holds");
                (ac ? have_ac : have_dc)[th] = true;
                i += 17 + cnt;
            }
        } else if (m == 0xdb) {
            for (uint32_t i = 0; i < nb;) {
                const uint32_t pq = body[i] >> 4, tq = body[i] & 15;
                if (pq > 1 || tq > 3 || i + 1 + 64 * (pq + 1) > nb)
                    return fail(kCorrupt, pos, "DQT");
                for (int nat = 0; nat < 64; nat++) {
                    const int k = jpegdec::zigzag_of(nat);
                    cur.q[tq][nat] = (uint16_t)(pq ? be16(body + i + 1 + 2 * k) : body[i + 1 + k]);
                }
                have_q[tq] = true;
                i += 1 + 64 * (pq + 1);
            }
        } else if (m == 0xdd) {
            if (ln != 4)
                return fail(kCorrupt, pos, "DRI");
            restart = be16(body);
        } else if (m == 0xdc) {
            return fail(kUnsupported, pos, "DNL");
        } else if (m == 0xee && nb >= 12 && std::memcmp(body, "Adobe", 5) == 0) {
            adobe = body[11];
        } else if (m == 0xda) {
            if (!have_frame || nb < 1 || nb != 4u + 2u * body[0] || body[0] < 1 || body[0] > g.nc)
                return fail(kCorrupt, pos, "SOS");
            out.scans.emplace_back();
            PScan& ps = out.scans.back();
            Scan& sc = ps.sc;
            std::memset(&sc, 0, sizeof(sc));
            const uint32_t ns = body[0];
            const uint32_t Ss = body[nb - 3], Se = body[nb - 2], Ah = body[nb - 1] >> 4, Al = body[nb - 1] & 15;
            if (Ss > 63 || Se > 63 || Se < Ss || (Ss == 0 && Se != 0) || (Ss > 0 && ns != 1) || Al > 13)
                return fail(kCorrupt, pos, "an illegal scan: its band, or an AC scan of several components");
            if (Ah != 0 && Ah != Al + 1)
                return fail(kCorrupt, pos, "an illegal scan: a refinement by other than one bit");
            sc.kind = (Ss ? kACFirst : kDCFirst) + (Ah ? 1u : 0u);
            sc.Ss = Ss, sc.Se = Se, sc.Al = Al, sc.ni = ns == 1;
            int before = -1;
            uint32_t pre = 0;
            for (uint32_t i = 0; i < ns; i++) {
                int c = -1;
                for (uint32_t k = 0; k < g.nc; k++)
                    if (comp_id[k] == body[1 + 2 * i])
                        c = (int)k;
                if (c < 0)
                    return fail(kCorrupt, pos, "SOS: no such component");
                if (c <= before)
                    return fail(kUnsupported, pos, "scan components out of order");
                before = c;
                const uint32_t td = body[2 + 2 * i] >> 4, ta = body[2 + 2 * i] & 15;
                if (td > 3 || ta > 3 || (sc.kind == kDCFirst && !have_dc[td]) || (sc.kind >= kACFirst && !have_ac[ta]))
                    return fail(kCorrupt, pos, "a table the scan names is missing");
                if (!latched[c]) {
                    if (comp_q[c] > 3 || !have_q[comp_q[c]])
                        return fail(kCorrupt, pos, "a table the scan names is missing");
                    std::memcpy(out.tab.q[c], cur.q[comp_q[c]], sizeof(cur.q[0]));
                    latched[c] = true;
                }
                for (uint32_t k = Ss; k <= Se; k++) {
                    if (Ah == 0 && bits[c][k] != -1)
                        return fail(kUnsupported, pos, "a coefficient's first scan comes twice");
                    if (Ah != 0 && bits[c][k] == -1)
                        return fail(kCorrupt, pos, "an illegal scan: a refinement of a coefficient whose first scan never came");
                    if (Ah != 0 && bits[c][k] != (int)Ah)
                        return fail(kCorrupt, pos, "an illegal scan: a refinement out of step");
                    bits[c][k] = (int8_t)Al;
                }
                sc.acsel = ta;
                if (ns == 1) {
                    const uint32_t wc = c ? g.cw : g.w, hc = c ? g.ch : g.h;
                    sc.comp0 = (uint32_t)c, sc.bw = (wc + 7) / 8;
                    sc.bps = 1, sc.nmcu = sc.nunits = sc.bw * ((hc + 7) / 8);
                    sc.dcsel = td;
                } else {
                    const uint32_t nbc = c ? 1u : g.ny;
                    for (uint32_t jc = 0; jc < nbc; jc++, sc.bps++) {
                        sc.dcsel |= td << (4 * sc.bps);
                        sc.ksel |= (c ? g.ny + (uint32_t)c - 1 : jc) << (4 * sc.bps);
                        sc.csel |= (jc | i << 2) << (4 * sc.bps);
                    }
                    sc.nbsel |= nbc << (4 * i), sc.presel |= pre << (4 * i);
                    pre += nbc;
                }
            }
            if (ns > 1)
                sc.nmcu = g.nmcu, sc.nunits = g.nmcu * sc.bps;
            ps.restart = restart;
            const uint32_t interval = restart ? restart : sc.nmcu;
            sc.nseg = (sc.nmcu + interval - 1) / interval, sc.ibl = interval * sc.bps;
            ps.tab = cur;
            pos += ln;
            // the walk over the scan's 0xFF bytes, as jpegdec_host.hpp's
            ps.scan_start = pos;
            ps.segoff.assign(1, 0u);
            uint64_t removed = 0, i = pos, j;
            uint8_t nx;
            for (;;) {
                const void* f = i < n ? std::memchr(d + i, 0xff, n - i) : nullptr;
                if (!f || (uint64_t)((const uint8_t*)f - d) + 1 >= n)
                    return fail(kCorrupt, n, "no EOI");
                j = (uint64_t)((const uint8_t*)f - d);
                nx = d[j + 1];
                if (nx == 0) {
                    removed++, i = j + 2;
                } else if (nx == 0xff) {
                    removed++, i = j + 1;
                } else if (nx >= 0xd0 && nx <= 0xd7) {
                    const uint64_t k = ps.segoff.size() - 1;
                    if (restart == 0 || (uint32_t)(nx - 0xd0) != (k & 7) || k + 1 >= sc.nseg)
                        return fail(kCorrupt, j, "a restart marker out of sequence");
                    ps.segoff.push_back((uint32_t)(j - pos - removed));
                    removed += 2, i = j + 2;
                } else {
                    break;
                }
            }
            if (nx == 0xdc)
                return fail(kUnsupported, j, "DNL");
            if (ps.segoff.size() != sc.nseg)
                return fail(kCorrupt, j, "restart markers missing");
            ps.scan_len = j - pos;
            if (ps.scan_len >= (1ull << 32) - 2 * jpegdec::kPiece)
                return fail(kUnsupported, pos, "a stuffed scan of 2^32 bytes");
            if ((ps.scan_len - removed) * 8 >= (1ull << 31))
                return fail(kUnsupported, pos, "a scan of 2^31 bits");
            ps.segoff.push_back((uint32_t)(ps.scan_len - removed));
            for (size_t k = 0; k + 1 < ps.segoff.size(); k++)
                if (ps.segoff[k + 1] <= ps.segoff[k])
                    return fail(kCorrupt, pos, "an empty segment");
            pos = j;  // the marker that ended the scan
            continue;
        }
        pos += ln;
    }
    if (g.nc == 3 && adobe == 0)
        return fail(kUnsupported, pos, "Adobe transform 0: RGB");
    // libjpeg smooths between blocks where a file stops short of full precision; the contract is the plain decode
    for (uint32_t c = 0; c < g.nc; c++)
        for (int k = 0; k < 64; k++)
            if (bits[c][k] != 0)
                return fail(kUnsupported, pos, "the scans leave coefficients unfinished");
    return kParsed;
}

// the first subsequence of every segment of a scan (nseg + 1 entries)
inline std::vector<uint32_t> sub_first(const PScan& p, uint32_t S)
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

}  // namespace jpegprog
}  // namespace v1c
