// jpegdec_batch_emul.hip -- TEST HARNESS: the batched JPEG decoder's decomposition on the CPU, workgroup by workgroup and lane by lane,
// over the product's own code: jpegdec_core.hpp (the arithmetic), jpegdec_host.hpp (the parse), jpegdec_batch.hpp (the work-list
// lookup, the flag rule, the chunks) and jpegdec_launch.hpp's workspace layout.  Every stage runs over a flat work list: a workgroup
// finds its file by file_of and its index within the file, as the k_jdecb_* kernels do; the rounds are shared by the files of a chunk,
// a file whose entry states stood still rests, and the last pass takes every file's own parity.
//
// Built by tests/test_jpegdec_batch_host.py (hipcc --cuda-host-only -O2 -shared -fPIC, into a temporary directory) and compared there
// with the restatement (tests/jpgdec_ref.py) file by file.  -DJDEC_MAIN: a stand-alone program for the sanitizer run.  -DJDEC_BREAK=1,
// 2, 3 breaks the design on purpose (DESIGN.md section 15 records what then fails): 1 -- two flag slots, so the slot a workgroup reads
// for "did my file change last round" is the one lane 0 clears; 2 -- the batch's last round as every file's parity in the last pass;
// 3 -- the work lists off by one workgroup at every other file boundary.  Not part of the product.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/vr180_remap.h"
#include "../../vr180_convert_amd/csrc/jpegdec_host.hpp"
#include "../../vr180_convert_amd/csrc/jpegdec_launch.hpp"

using namespace v1c::jpegdec;

#ifndef JDEC_BREAK
#define JDEC_BREAK 0
#endif

namespace {

struct File {
    Parsed ps;
    int status = 0;  // 0: decoded, 1: unsupported, 2: corrupt by the parse, 3: corrupt by the last pass
    uint32_t S = 0, nsub = 0, pieces = 0, scan_len = 0;
    std::vector<uint32_t> subfirst, u, count, drop, dcd;
    std::vector<uint64_t> dropoff, first, dcoff;
    std::vector<uint8_t> scan, plane[3];
    std::vector<State> ex[2], last, entry;
    std::vector<int16_t> coef;
    TablePair tp;
    uint32_t flags[kFlagWords] = {0, 0, 0, 0xffffffffu};
    uint32_t rounds = 0;
    uint64_t workspace = 0;
    uint8_t* out = nullptr;
    int out_cn = 3;
};

struct SubE {
    uint32_t k, start, end, E;
    bool first, last;
};

SubE sub_of(const File& r, uint32_t i)
{
    uint32_t lo = 0, hi = r.ps.g.nseg - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (r.subfirst[mid] <= i)
            lo = mid;
        else
            hi = mid - 1;
    }
    SubE s;
    s.k = lo, s.E = 8 * r.ps.segoff[lo + 1];
    const uint32_t j = i - r.subfirst[lo];
    s.start = 8 * r.ps.segoff[lo] + j * r.S;
    s.end = std::min(s.start + r.S, s.E);
    s.first = j == 0, s.last = i + 1 == r.subfirst[lo + 1];
    return s;
}

uint32_t slot(uint32_t r)
{
    return JDEC_BREAK == 1 ? r & 1u : r % kRoundSlots;
}

bool active(const File& f, uint32_t r)
{
#if JDEC_BREAK == 1
    return r == 1 || (r <= f.nsub + 1 && f.flags[slot(r - 1)] != 0);
#else
    return file_active(f.flags, r, f.nsub);
#endif
}

uint64_t groups(uint64_t n, uint32_t per)
{
    return (n + per - 1) / per;
}

// the workgroups of file f in every list
void work_of(const File& f, uint64_t* w)
{
    const Geom& g = f.ps.g;
    w[kByPiece] = groups(f.pieces, 256), w[kBySub] = groups(f.nsub, 256), w[kByBlock] = groups(g.nblocks, 256);
    w[kByTile] = groups(g.nblocks, 32), w[kByPixel] = groups((uint64_t)((g.w + 3) / 4) * g.h, 256);
}

struct Chunk {
    std::vector<File*> files;
    std::vector<uint32_t> first;  // kWorkLists x (n + 1)
    uint32_t n() const { return (uint32_t)files.size(); }

    void list(int l)
    {
        uint32_t* fl = first.data() + (size_t)l * (n() + 1);
        fl[0] = 0;
        for (uint32_t f = 0; f < n(); f++) {
            uint64_t w[kWorkLists];
            work_of(*files[f], w);
            fl[f + 1] = fl[f] + (uint32_t)w[l];
        }
#if JDEC_BREAK == 3
        for (uint32_t f = 1; f < n(); f += 2)
            fl[f] += 1;
#endif
    }

    // one launch: every workgroup of list l finds its file and its index within the file
    template <class Body>
    void launch(int l, Body body)
    {
        const uint32_t* fl = first.data() + (size_t)l * (n() + 1);
        for (uint32_t wg = 0; wg < fl[n()]; wg++) {
            const uint32_t f = file_of(fl, n(), wg);
            body(*files[f], wg - fl[f]);
        }
    }
};

void prepare(File& f, const uint8_t* file)
{
    const Geom& g = f.ps.g;
    f.subfirst = sub_first(f.ps, f.S);
    f.nsub = f.subfirst.back();
    f.scan_len = (uint32_t)f.ps.scan_len, f.pieces = (f.scan_len + kPiece - 1) / kPiece;
    f.scan.assign(((size_t)f.pieces + 1) * kPiece, 0);
    std::memcpy(f.scan.data(), file + f.ps.scan_start, (size_t)f.scan_len + 2);
    f.drop.assign(f.pieces, 0), f.dropoff.assign((size_t)f.pieces + 1, 0);
    f.u.assign(f.ps.segoff.back() / 4 + 3, 0);
    f.ex[0].assign(f.nsub, State{0, 0}), f.ex[1].assign(f.nsub, State{0, 0}), f.last.assign(f.nsub, State{0, 0});
    f.count.assign(f.nsub, 0), f.first.assign((size_t)f.nsub + 1, 0), f.entry.assign(f.nsub, State{0, 0});
    f.coef.assign((size_t)g.nblocks * 64, 0);
    f.dcd.assign(g.nblocks, 0), f.dcoff.assign((size_t)g.nblocks + 1, 0);
    for (uint32_t c = 0; c < g.nc; c++)
        f.plane[c].assign((size_t)plane_pitch(g, c) * plane_rows(g, c), 0);
    f.tp = table_pair(g, f.ps.tab.dc, f.ps.tab.ac);
    f.workspace = layout_of(f.ps, f.nsub).bytes;
}

void scan_of(const std::vector<uint32_t>& in, std::vector<uint64_t>& out)
{
    for (size_t i = 0; i < in.size(); i++)
        out[i + 1] = out[i] + in[i];
}

// one chunk; returns its rounds
uint32_t run_chunk(Chunk& c)
{
    c.first.assign((size_t)kWorkLists * (c.n() + 1), 0);
    for (int l = 0; l < kWorkLists; l++)
        c.list(l);
    // unstuffing
    c.launch(kByPiece, [](File& f, uint32_t wg) {
        for (uint32_t lane = 0; lane < 256; lane++) {
            const uint32_t p = wg * 256u + lane;
            if (p >= f.pieces)
                continue;
            uint32_t prev = p ? f.scan[(size_t)p * kPiece - 1] : 0u, n = 0;
            for (int j = 0; j < kPiece; j++) {
                const size_t at = (size_t)p * kPiece + j;
                n += (at < f.scan_len && dropped(prev, f.scan[at], f.scan[at + 1])) ? 1u : 0u;
                prev = f.scan[at];
            }
            f.drop[p] = n;
        }
    });
    for (File* f : c.files)
        scan_of(f->drop, f->dropoff);
    c.launch(kByPiece, [](File& f, uint32_t wg) {
        for (uint32_t lane = 0; lane < 256; lane++) {
            const uint32_t p = wg * 256u + lane;
            if (p >= f.pieces)
                continue;
            uint8_t* dst = (uint8_t*)f.u.data() + ((uint64_t)p * kPiece - f.dropoff[p]);
            uint32_t prev = p ? f.scan[(size_t)p * kPiece - 1] : 0u;
            for (int j = 0; j < kPiece; j++) {
                const size_t at = (size_t)p * kPiece + j;
                if (at < f.scan_len && !dropped(prev, f.scan[at], f.scan[at + 1]))
                    *dst++ = f.scan[at];
                prev = f.scan[at];
            }
        }
    });
    // the rounds, shared
    c.launch(kBySub, [](File& f, uint32_t wg) {
        for (uint32_t lane = 0; lane < 256; lane++) {
            const uint32_t i = wg * 256u + lane;
            if (i >= f.nsub)
                continue;
            f.ex[0][i] = State{sub_of(f, i).end, 0u};
            f.last[i] = State{0xffffffffu, 0xffffffffu};
            f.count[i] = 0;
        }
    });
    uint32_t r = 0, open = c.n(), most = 0;
    for (File* f : c.files)
        most = std::max(most, f->nsub);
    while (open) {
        r++;
        c.launch(kBySub, [r](File& f, uint32_t wg) {
            if (!active(f, r)) {
                if (wg == 0)
                    f.flags[slot(r)] = 0;
                return;
            }
            const std::vector<State>& in = f.ex[(r - 1) & 1];
            std::vector<State>& out = f.ex[r & 1];
            for (uint32_t lane = 0; lane < 256; lane++) {
                const uint32_t i = wg * 256u + lane;
                if (i == 0)
                    f.flags[slot(r + 1)] = 0;
                if (i >= f.nsub)
                    continue;
                const SubE s = sub_of(f, i);
                const State e = s.first ? State{s.start, 0u} : in[i - 1];
                if (e == f.last[i]) {
                    out[i] = in[i];
                    continue;
                }
                State x = e;
                f.count[i] = decode_span<false>(f.u.data(), f.tp, f.ps.g.bpm, x, s.end, s.E, nullptr, 0, 0, nullptr);
                f.last[i] = e, out[i] = x;
                if (!s.last && !(x == in[i]))
                    f.flags[slot(r)] = 1;
            }
        });
        // the host between two rounds: one copy of all the flags; a file is done at its first quiet round, or at its bound
        for (File* f : c.files)
            if (!f->rounds && (f->flags[slot(r)] == 0 || r > f->nsub)) {
                f->rounds = r;
                open--;
            }
        if (r > most)
            break;
    }
    // the last pass, every file by its own parity
    for (File* f : c.files)
        scan_of(f->count, f->first);
    c.launch(kBySub, [r](File& f, uint32_t wg) {
        const Geom& g = f.ps.g;
        const uint32_t par = JDEC_BREAK == 2 ? r : f.rounds;
        for (uint32_t lane = 0; lane < 256; lane++) {
            const uint32_t i = wg * 256u + lane;
            if (i >= f.nsub)
                continue;
            const SubE s = sub_of(f, i);
            State e = s.first ? State{s.start, 0u} : f.ex[par & 1][i - 1];
            f.entry[i] = e;
            const uint32_t i0 = f.subfirst[s.k], b0 = s.k * g.ibl, bq = std::min(b0 + g.ibl, g.nblocks);
            const uint64_t done = f.first[i] - f.first[i0];
            const uint32_t b = done < bq - b0 ? b0 + (uint32_t)done : bq;
            uint32_t err = 0xffffffffu;
            decode_span<true>(f.u.data(), f.tp, g.bpm, e, s.end, s.E, f.coef.data(), b, bq, &err);
            if (s.first && f.first[f.subfirst[s.k + 1]] - f.first[i0] != bq - b0)
                err = std::min(err, s.start);
            f.flags[kErrSlot] = std::min(f.flags[kErrSlot], err);
        }
    });
    for (File* f : c.files)
        if (f->flags[kErrSlot] != 0xffffffffu)
            f->status = 3;
    // pixels: the workgroups of a file the last pass refused return at once
    c.launch(kByBlock, [](File& f, uint32_t wg) {
        if (f.flags[kErrSlot] != 0xffffffffu)
            return;
        for (uint32_t lane = 0; lane < 256; lane++) {
            const uint32_t b = wg * 256u + lane;
            if (b >= f.ps.g.nblocks)
                continue;
            uint32_t pos, pos0;
            dc_pos(f.ps.g, b, pos, pos0);
            f.dcd[pos] = (uint32_t)(int)f.coef[(size_t)b * 64];
        }
    });
    for (File* f : c.files)
        if (!f->status)
            scan_of(f->dcd, f->dcoff);
    c.launch(kByTile, [](File& f, uint32_t wg) {
        const Geom& g = f.ps.g;
        if (f.flags[kErrSlot] != 0xffffffffu)
            return;
        for (uint32_t blk = 0; blk < 32; blk++) {
            const uint32_t b = wg * 32u + blk;
            if (b >= g.nblocks)
                continue;
            const BlockPos pos = block_pos(g, b);
            const uint16_t* q = f.ps.tab.q[g.tq[pos.comp]];
            int tile[8][8];
            for (int col = 0; col < 8; col++) {
                int d[8];
                for (int i = 0; i < 8; i++)
                    d[i] = dequantise(f.coef[(size_t)b * 64 + zigzag_of(i * 8 + col)], q[i * 8 + col]);
                if (col == 0) {
                    uint32_t at, at0;
                    dc_pos(g, b, at, at0);
                    d[0] = dequantise((int16_t)(uint32_t)(f.dcoff[at + 1] - f.dcoff[at0]), q[0]);
                }
                idct_pass<11>(d);
                for (int i = 0; i < 8; i++)
                    tile[i][col] = d[i];
            }
            for (int row = 0; row < 8; row++) {
                int d[8];
                for (int col = 0; col < 8; col++)
                    d[col] = tile[row][col];
                idct_pass<18>(d);
                for (int col = 0; col < 8; col++)
                    f.plane[pos.comp][(size_t)(pos.y0 + row) * plane_pitch(g, pos.comp) + pos.x0 + col] = (uint8_t)clamp255(d[col] + 128);
            }
        }
    });
    c.launch(kByPixel, [](File& f, uint32_t wg) {
        const Geom& g = f.ps.g;
        if (f.flags[kErrSlot] != 0xffffffffu)
            return;
        const uint32_t wq = (g.w + 3) / 4;
        for (uint32_t lane = 0; lane < 256; lane++) {
            const uint64_t idx = (uint64_t)wg * 256u + lane;
            if (idx >= (uint64_t)wq * g.h)
                continue;
            const uint32_t y = (uint32_t)(idx / wq), x0 = (uint32_t)(idx - (uint64_t)y * wq) * 4;
            for (uint32_t x = x0; x < std::min(x0 + 4, g.w); x++) {
                uint8_t* px = f.out + ((size_t)y * g.w + x) * f.out_cn;
                const int lum = f.plane[0][(size_t)y * plane_pitch(g, 0) + x];
                if (g.nc == 1) {
                    for (int k = 0; k < f.out_cn; k++)
                        px[k] = (uint8_t)lum;
                } else {
                    ycc_to_bgr(lum, chroma_sample(f.plane[1].data(), plane_pitch(g, 1), g, x, y),
                               chroma_sample(f.plane[2].data(), plane_pitch(g, 1), g, x, y), px);
                }
            }
        }
    });
    return r;
}

// the whole batch: the parse of every file first, then the chunks of the files it accepted; batch: rounds, chunks
void run_batch(std::vector<File>& files, const uint8_t* const* data, const uint64_t* sizes, uint32_t S, uint64_t budget, uint32_t* batch)
{
    std::vector<File*> good;
    std::vector<uint64_t> bytes, wgs;
    for (size_t i = 0; i < files.size(); i++) {
        File& f = files[i];
        f.S = S;
        f.status = (int)parse(data[i], sizes[i], f.ps);
        if (f.status)
            continue;
        prepare(f, data[i]);
        uint64_t w[kWorkLists];
        work_of(f, w);
        good.push_back(&f), bytes.push_back(f.workspace + sizeof(Args) + 1024), wgs.push_back(*std::max_element(w, w + kWorkLists));
    }
    batch[0] = batch[1] = 0;
    uint32_t at = 0;
    for (uint32_t end : chunk_ends(bytes, wgs, budget ? budget : kDefaultBatchWorkspace)) {
        Chunk c;
        c.files.assign(good.begin() + at, good.begin() + end);
        batch[0] += run_chunk(c), batch[1]++;
        at = end;
    }
}

}  // namespace

extern "C" {

// info: height, width, components, h_samp, v_samp, restart interval, segments, blocks
int jdecb_info(const uint8_t* file, uint64_t size, int32_t* info)
{
    Parsed p;
    const ParseResult r = parse(file, size, p);
    if (r != kParsed)
        return (int)r;
    const int32_t v[8] = {(int32_t)p.g.h, (int32_t)p.g.w, (int32_t)p.g.nc, (int32_t)p.g.hs, (int32_t)p.g.vs, (int32_t)p.restart,
                          (int32_t)p.g.nseg, (int32_t)p.g.nblocks};
    std::memcpy(info, v, sizeof(v));
    return 0;
}

// the workspace the product gives the file at S bits per subsequence; 0 for a file the parse refuses
uint64_t jdecb_workspace(const uint8_t* file, uint64_t size, uint32_t S)
{
    Parsed p;
    if (parse(file, size, p) != kParsed)
        return 0;
    return layout_of(p, sub_first(p, S).back()).bytes + sizeof(Args) + 1024;  // (with its share of a chunk's head, as the product counts)
}

// Per file i: status[i] (0 decoded, 1 unsupported, 2 corrupt by the parse, 3 corrupt by the last pass); reports[4 i ..]: segments,
// subsequences, rounds, error bit; error_pos[i]: the parse's byte; and, where the file decoded, coef[i]: nblocks x 64 (the DC a
// difference), states[i]: 3 words per subsequence (p, z, c), counts[i]: one, both of caps[i] subsequences, pixels[i]: h x w x 3 dense.
// batch: rounds, chunks.  Returns 0, or -2 where a file has more subsequences than its cap.
int jdecb_decode(int n, const uint8_t* const* data, const uint64_t* sizes, uint32_t S, uint64_t budget, int16_t* const* coef,
                 uint32_t* const* states, uint32_t* const* counts, const uint32_t* caps, uint32_t* reports, uint64_t* error_pos,
                 uint8_t* const* pixels, int* status, uint32_t* batch)
{
    std::vector<File> files((size_t)n);
    for (int i = 0; i < n; i++)
        files[i].out = pixels[i];
    run_batch(files, data, sizes, S ? S : kDefaultSubseqBits, budget, batch);
    for (int i = 0; i < n; i++) {
        const File& f = files[i];
        status[i] = f.status, error_pos[i] = f.ps.error_pos;
        if (f.status == 1 || f.status == 2)
            continue;
        uint32_t* rep = reports + 4 * i;
        rep[0] = f.ps.g.nseg, rep[1] = f.nsub, rep[2] = f.rounds, rep[3] = f.flags[kErrSlot];
        if (f.status)
            continue;
        if (f.nsub > caps[i])
            return -2;
        std::memcpy(coef[i], f.coef.data(), f.coef.size() * 2);
        for (uint32_t k = 0; k < f.nsub; k++) {
            states[i][3 * k] = f.entry[k].p, states[i][3 * k + 1] = f.entry[k].zc & 255u, states[i][3 * k + 2] = f.entry[k].zc >> 8;
            counts[i][k] = f.count[k];
        }
    }
    return 0;
}

}

#ifdef JDEC_MAIN
// Decodes the files named on the command line as batches -- all of them, the same in reverse, and all of them under a budget that
// cuts the list into several chunks -- at two subsequence sizes, and prints one line per file and batch.  The exit status is 0 unless
// a file cannot be read or the batches disagree about a file.
int main(int argc, char** argv)
{
    std::vector<std::vector<uint8_t>> data;
    for (int i = 1; i < argc; i++) {
        std::FILE* f = std::fopen(argv[i], "rb");
        if (!f)
            return 1;
        std::vector<uint8_t> d;
        uint8_t buf[4096];
        for (size_t n; (n = std::fread(buf, 1, sizeof(buf), f)) > 0;)
            d.insert(d.end(), buf, buf + n);
        std::fclose(f);
        std::vector<uint8_t> exact(d.begin(), d.end());  // (an exact-size heap copy: a read one byte past the file is a report)
        exact.shrink_to_fit();
        data.push_back(std::move(exact));
    }
    const size_t n = data.size();
    int bad = 0;
    for (uint32_t S : {256u, 1024u}) {
        std::vector<unsigned long> want(n);
        std::vector<int> want_status(n);
        for (int mode = 0; mode < 3; mode++) {
            std::vector<size_t> order(n);
            for (size_t i = 0; i < n; i++)
                order[i] = mode == 1 ? n - 1 - i : i;
            std::vector<const uint8_t*> ptr(n);
            std::vector<uint64_t> sizes(n);
            std::vector<std::vector<uint8_t>> px(n);
            std::vector<File> files(n);
            uint64_t largest = 0;
            for (size_t i = 0; i < n; i++) {
                const std::vector<uint8_t>& d = data[order[i]];
                ptr[i] = d.data(), sizes[i] = d.size();
                Parsed p;
                if (parse(d.data(), d.size(), p) == kParsed) {
                    px[i].assign((size_t)p.g.h * p.g.w * 3, 0);
                    largest = std::max<uint64_t>(largest, layout_of(p, sub_first(p, S).back()).bytes + sizeof(Args) + 1024);
                }
                files[i].out = px[i].data();
            }
            uint32_t batch[2];
            run_batch(files, ptr.data(), sizes.data(), S, mode == 2 ? 3 * largest : 0, batch);
            for (size_t i = 0; i < n; i++) {
                unsigned long sum = 0;
                if (files[i].status == 0)
                    for (uint8_t v : px[i])
                        sum += v;
                std::printf("%s S=%u mode=%d rc=%d rounds=%u sum=%lu\n", argv[1 + order[i]], S, mode, files[i].status, files[i].rounds, sum);
                if (mode == 0)
                    want[order[i]] = sum, want_status[order[i]] = files[i].status;
                else if (want[order[i]] != sum || want_status[order[i]] != files[i].status)
                    bad = 1;
            }
            std::printf("batch S=%u mode=%d rounds=%u chunks=%u\n", S, mode, batch[0], batch[1]);
        }
    }
    return bad;
}
#endif
