"""The boundary cases of the lossless JPEG composer, shared by the host half (tests/test_jpegxf_host.py) and the GPU half
(tests/test_gpu_jpegxf.py).  A case is a list of source files and a list of outputs (jpgxf_ref's form: regions in MCUs with a source
and a transform each).  The sources are jpgxc_cases' (Pillow, or the encoder's restatement for any restart interval); nothing is larger
than a few hundred blocks.  The restatement of each case is computed once and shared."""
from __future__ import annotations

import functools
import struct

import numpy as np

import jpg_cases as PC
import jpgdec_cases as JC
import jpgxc_cases as K
import jpgxf_ref as F

KINDS = K.KINDS
ALL = list(range(8))
PLAIN = [0, 1, 2, 3]  # the codes a 4:2:2 file takes


def codes_of(kind):
    return PLAIN if kind == "422" else ALL


def whole(src, code, **kw):
    return F.transform_output(src, code, **kw)


def dqt16_asymmetric(data, value=300):
    """the file with 16-bit quantisation tables (SOF1) whose entry of horizontal frequency 1, vertical 0 is ``value``: tables that differ
    from their transpose in an entry above 255"""
    out = JC.dqt16_sof1(data)
    for m, a, e in reversed(JC.header_segments(out)):
        if m == 0xDB:
            body = bytearray(out[a + 4:e])
            for i in range(0, len(body), 129):
                body[i + 1 + 2:i + 1 + 4] = struct.pack(">H", value)  # zigzag position 1
            out = out[:a] + JC.segment(0xDB, bytes(body)) + out[e:]
    return out


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    """name: (files, outputs)"""
    c = {}

    def add(name, datas, make):
        srcs = F.sources_of(list(datas))
        c[name] = (tuple(datas), make(srcs))

    for k, kind in enumerate(KINDS):
        codes = codes_of(kind)
        # the smallest images under every code, one output each: the mirror of a single column and of a single row
        for mx, my in ((1, 1), (1, 2), (2, 1), (3, 2)):
            add(f"all_codes_{mx}x{my}_{kind}", [K._file(kind, mx, my, 500 + 10 * mx + my + k)], lambda s, codes=codes: [whole(s[0], t) for t in codes])
        # sources with restart markers every 1, 2 and 7 MCUs; outputs with every MCU an interval, a row, none
        for n, (r, out_r) in enumerate(((1, 0), (2, 1), (7, None))):
            add(f"source_dri{r}_{kind}", [K._file(kind, 5, 3, 540 + 10 * r + k, restart=r)],
                lambda s, out_r=out_r, codes=codes, n=n: [whole(s[0], codes[(n + 1 + j) % len(codes)], restart_mcus=out_r) for j in range(2)]
                + [dict(width=3 * s[0].mw, height=2 * s[0].mh, restart_mcus=out_r, regions=[(0, codes[-1], 1, 0, *((2, 3) if codes[-1] & 4 else (3, 2)), 0, 0)])])
        # optimised and plain outputs in one call
        add(f"optimize_mixed_{kind}", [K._file(kind, 4, 2, 580 + k, noise=True, quality=95)],
            lambda s, codes=codes: [whole(s[0], codes[-1], optimize=True), whole(s[0], 3), whole(s[0], 1, optimize=True, restart_mcus=0)])
        # two sources side by side; the right eye upside-down; four sources as a 2 x 2 mosaic with a code each
        eyes = [K._file(kind, 3, 2, 600 + 10 * j + k, restart=(None, 2)[j]) for j in range(2)]
        add(f"join_{kind}", eyes, lambda s: [F.join_output(s[0], s[1])])
        add(f"join_right_rot180_{kind}", eyes, lambda s: [F.join_output(s[0], s[1], None, "rot180", optimize=True)])
        four = [K._file(kind, 2, 2, 640 + 10 * j + k, restart=(None, 1, 3, None)[j]) for j in range(4)]
        add(f"mosaic_{kind}", four, lambda s: [dict(width=4 * s[0].mw, height=4 * s[0].mh,
                                                    regions=[(j, (3, 0, 1, 2)[j], 0, 0, 2, 2, 2 * (j % 2), 2 * (j // 2)) for j in range(4)])])
        # a partial last column and row: kept where nothing mirrors them, trimmed off where a mirror needs whole MCUs
        part = K._file(kind, 3, 2, 680 + k, dw=-3, dh=-5)
        add(f"partial_kept_{kind}", [part], lambda s, kind=kind: [whole(s[0], 0)] + ([whole(s[0], 4)] if kind != "422" else []))
        add(f"partial_trimmed_{kind}", [part], lambda s, codes=codes: [whole(s[0], t, trim=True) for t in codes[1:]])
        add(f"join_trimmed_{kind}", [part, part], lambda s: [F.join_output(s[0], s[1], "flip_v", "rot180", trim=True)])
    # outputs of 31 ... 33 and 255 ... 258 blocks: the gather's workgroup of 32 blocks and the encoder stages' of 256; the last launch's edge
    for n in (31, 32, 33, 255, 256, 257, 258):
        add(f"blocks_{n}", [K._file("gray", n, 1, 700 + n, restart=5)], lambda s: [whole(s[0], 3), whole(s[0], 5, restart_mcus=4), whole(s[0], 1, optimize=True)])
    add("blocks_258_420", [K._file("420", 43, 1, 721)], lambda s: [whole(s[0], 1), whole(s[0], 6), whole(s[0], 7, restart_mcus=0)])
    add("blocks_258_444", [K._file("444", 43, 2, 722, restart=9)], lambda s: [whole(s[0], 2), whole(s[0], 4)])
    add("blocks_256_422", [K._file("422", 32, 2, 723, restart=11)], lambda s: [whole(s[0], 3, restart_mcus=7)])
    # the largest coefficients the encoder's tables code: DCs of -1024 and 1023 next to each other, ACs of +-1023 at odd frequencies
    # (zigzag positions 1: u = 1; 2: v = 1; 4: u = v = 1), which the mirrors negate
    limits = K._coded({(0, 0): 1023, (1, 0): -1024, (2, 0): 1023, (0, 1): 1023, (0, 2): -1023, (1, 1): -1023, (1, 4): 1023, (2, 2): 1023, (2, 63): -1023}, 3)
    add("coefficient_limits", [limits], lambda s: [whole(s[0], t, restart_mcus=r) for t, r in zip(ALL, (0, 1, None, 0, 1, None, 0, 1))])
    # 16-bit quantisation tables that differ from their transpose; Pillow's tables, which do too; one table for all components
    wide = dqt16_asymmetric(JC.pillow(PC.smooth(33, 47, 3, 731), 90, "420"))
    add("dqt16_transposed", [wide], lambda s: [whole(s[0], 4), whole(s[0], 0), whole(s[0], 5, trim=True)])
    add("asymmetric_tables_444", [JC.pillow(PC.smooth(24, 40, 3, 732), 75, "444")], lambda s: [whole(s[0], 6), whole(s[0], 7)])
    # symmetric tables (quality 100: all ones): transposed and untransposed regions in one output, from two files
    ones = [JC.pillow(PC.smooth(32, 32, 3, 733 + j), 100, "420") for j in range(2)]
    add("mixed_transpose_symmetric_tables", ones, lambda s: [dict(width=64, height=32, regions=[(0, 5, 0, 0, 2, 2, 0, 0), (1, 2, 0, 0, 2, 2, 2, 0)])])
    # a region of a larger source, transposed to a rectangle that is not square, beside an untransformed one of another source
    add("transposed_rectangle", [JC.pillow(PC.smooth(48, 64, 1, 735), 100), JC.pillow(PC.smooth(24, 16, 1, 736), 100)],
        lambda s: [dict(width=40, height=24, restart_mcus=2, regions=[(0, 6, 2, 1, 3, 2, 0, 0), (1, 0, 0, 0, 2, 3, 2, 0), (0, 7, 5, 3, 3, 1, 4, 0)])])
    return c


@functools.lru_cache(maxsize=None)
def reference(name) -> tuple:
    """the restatement's files of a case"""
    datas, outputs = cases()[name]
    return tuple(F.compose(list(datas), outputs))


def out_of_range() -> dict:
    """name: (files, outputs): valid files with a coefficient the encoder's tables do not code, refused after the decode"""
    ok = K._coded({(0, 0): 5, (1, 3): 7}, 2)
    outs = [dict(width=32, height=8, regions=[(0, 1, 0, 0, 2, 1, 0, 0), (1, 2, 0, 0, 2, 1, 2, 0)])]
    return {
        "dc_1024_second_source": ([ok, K._coded({(0, 0): 1024, (1, 0): 1024}, 2)], outs),
        "ac_1024_first_source": ([K._coded({(1, 9): 1024}, 2), ok], outs),
        "ac_minus_1024_negated": ([K._coded({(1, 1): -1024}, 2), ok], outs),
    }


@functools.lru_cache(maxsize=None)
def refused() -> dict:
    """name: (files, outputs, the exception of jpgxf_ref)"""
    img = PC.smooth(48, 64, 3, 800)
    a420 = JC.pillow(img, 90, "420")       # 4 x 3 MCUs
    b420 = JC.pillow(img[::-1], 90, "420")
    q75 = JC.pillow(img, 75, "420")
    a444 = JC.pillow(img, 90, "444")
    a422 = JC.pillow(img, 90, "422")       # 4 x 6 MCUs
    gray = JC.pillow(img[..., 0], 90)
    whole = [(0, 0, 0, 0, 4, 3, 0, 0)]
    return {
        "other_sampling": ([a420, a444], [dict(width=64, height=48, regions=whole)], F.Unsupported),
        "other_components": ([a444, gray], [dict(width=64, height=48, regions=[(0, 0, 0, 0, 8, 6, 0, 0)])], F.Unsupported),
        "progressive_second_source": ([a420, JC.pillow(img, 90, "420", progressive=True)], [dict(width=64, height=48, regions=whole)], F.Unsupported),
        "transposed_422": ([a422], [dict(width=48, height=64, regions=[(0, 4, 0, 0, 4, 6, 0, 0)])], F.Unsupported),
        "other_tables": ([a420, q75], [dict(width=128, height=48, regions=whole + [(1, 0, 0, 0, 4, 3, 4, 0)])], F.Unsupported),
        "transposed_beside_plain_asymmetric_tables": ([a420, b420], [dict(width=112, height=64, regions=[(0, 5, 0, 0, 4, 3, 0, 0), (1, 0, 0, 0, 4, 3, 3, 0)])],
                                                      F.Unsupported),
        "overlapping_placed_rectangles": ([a420], [dict(width=64, height=64, regions=[(0, 4, 0, 0, 4, 3, 0, 0), (0, 4, 0, 0, 4, 2, 2, 0)])], F.Unsupported),
        "uncovered_mcus": ([a420, b420], [dict(width=128, height=48, regions=whole + [(1, 3, 0, 0, 3, 3, 4, 0)])], F.Invalid),
        "region_outside_source": ([a420, b420], [dict(width=128, height=48, regions=whole + [(1, 1, 1, 0, 4, 3, 4, 0)])], F.Invalid),
        # 4 x 3 MCUs transposed are 3 x 4: they do not fit the 4 x 3 they came from
        "placed_rectangle_outside_output": ([a420], [dict(width=64, height=48, regions=[(0, 4, 0, 0, 4, 3, 0, 0)])], F.Invalid),
        "no_such_source": ([a420, b420], [dict(width=64, height=48, regions=[(2, 0, 0, 0, 4, 3, 0, 0)])], F.Invalid),
        "negative_source": ([a420], [dict(width=64, height=48, regions=[(-1, 0, 0, 0, 4, 3, 0, 0)])], F.Invalid),
        "transform_8": ([a420], [dict(width=64, height=48, regions=[(0, 8, 0, 0, 4, 3, 0, 0)])], F.Invalid),
        "five_sources": ([a420] * 5, [dict(width=64, height=48, regions=whole)], F.Invalid),
        "no_regions": ([a420], [dict(width=64, height=48, regions=[])], F.Invalid),
        "seventeen_regions": ([a420], [dict(width=16 * 17, height=16, regions=[(0, 1, 0, 0, 1, 1, i, 0) for i in range(17)])], F.Invalid),
        "restart_too_large": ([a420], [dict(width=64, height=48, restart_mcus=65536, regions=whole)], F.Invalid),
    }


def corrupt() -> dict:
    """name: (files, outputs, whether the parse alone finds it): a sound first source and a damaged second one"""
    import jpgdec_ref as D

    out = {}
    for name, (data, by_parse) in JC.corrupt_cases().items():
        try:
            s = D.parse(data)
            cn, sub = s.nc, {(1, 1): "444", (2, 1): "422", (2, 2): "420"}[(s.hs, s.vs)]
        except (D.Corrupt, D.Unsupported, KeyError):
            cn, sub = 1, "444"
        good = JC.pillow(PC.smooth(32, 32, cn, 810), 90, sub)  # (of the damaged file's components and sampling: only the damage refuses the call)
        g = D.parse(good)
        out[name] = ([good, data], [dict(width=32, height=32, regions=[(0, 3, 0, 0, g.mcux, g.mcuy, 0, 0)])], by_parse)
    return out
