"""The boundary cases of the lossless JPEG transcoder, shared by the host half (tests/test_jpegxc_host.py: the restatement against an
independent decoder, the product's host build against the restatement) and the GPU half (tests/test_gpu_jpegxc.py,
tests/test_gpu_jpegxc_edges.py: the kernels against the same bytes).  A case is a source file and a list of outputs (jpgxc_ref's form:
regions in MCUs).  Sources are written by Pillow (any tables, no restart markers) or by the encoder's restatement (any restart
interval).  Every case is a fraction of a second; the restatement of each is computed once and shared."""
from __future__ import annotations

import functools

import numpy as np

import jpg_cases as PC
import jpg_ref as R
import jpgdec_cases as JC
import jpgdec_ref as D
import jpgxc_ref as X

KINDS = {"gray": (1, "420", 8, 8), "444": (3, "444", 8, 8), "422": (3, "422", 16, 8), "420": (3, "420", 16, 16)}  # channels, sampling, MCU width, height


def _file(kind, mx, my, seed, dw=0, dh=0, restart=None, quality=90, noise=False):
    """a source of mx x my MCUs, its size dw / dh pixels off the full MCUs (negative: a partial last column / row)"""
    cn, sub, m, n = KINDS[kind]
    h, w = my * n + dh, mx * m + dw
    img = (PC.noise if noise else PC.smooth)(h, w, cn, seed)
    if restart is None:
        return JC.pillow(img, quality, sub)
    if sub == "422":  # (the encoder's restatement writes no 4:2:2: Pillow's restart interval, in MCUs)
        return JC.pillow(img, quality, sub, restart_marker_blocks=restart)
    return R.encode(img, quality, sub, restart)


def _whole(src):
    return X.crop_output(src)


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    """name: (file, outputs)"""
    c = {}

    def add(name, data, make):
        src = X.Source(data)
        c[name] = (data, make(src))

    for k, kind in enumerate(KINDS):
        m, n = KINDS[kind][2:]
        # the smallest images: one MCU, 2 x 2 and 3 x 2, coded again as a whole; a swap whose halves are one MCU wide; crops of a column
        add(f"whole_1x1_{kind}", _file(kind, 1, 1, 100 + k), lambda s: [_whole(s)])
        add(f"whole_2x2_{kind}", _file(kind, 2, 2, 110 + k), lambda s: [_whole(s)])
        add(f"whole_3x2_{kind}", _file(kind, 3, 2, 120 + k, restart=2), lambda s: [_whole(s)])
        add(f"swap_2x2_{kind}", _file(kind, 2, 2, 130 + k), lambda s: [X.swap_output(s)])
        add(f"split_2x1_{kind}", _file(kind, 2, 1, 140 + k), lambda s: X.split_outputs(s))
        add(f"first_column_{kind}", _file(kind, 3, 2, 150 + k), lambda s, m=m, n=n: [X.crop_output(s, (0, 0, m, 2 * n))])
        add(f"last_column_{kind}", _file(kind, 3, 2, 160 + k), lambda s, m=m, n=n: [X.crop_output(s, (2 * m, 0, m, 2 * n))])
        # sources of mcu * k + 1 and mcu * k - 1 pixels: the partial last column and row, alone and with their neighbours
        add(f"plus1_partial_column_{kind}", _file(kind, 3, 2, 170 + k, dw=1, dh=1), lambda s, m=m, n=n: [X.crop_output(s, (3 * m, 0, 1, 2 * n + 1))])
        add(f"plus1_partial_row_{kind}", _file(kind, 3, 2, 180 + k, dw=1, dh=1), lambda s, m=m, n=n: [X.crop_output(s, (0, 2 * n, 3 * m + 1, 1))])
        add(f"minus1_last_two_columns_{kind}", _file(kind, 3, 2, 190 + k, dw=-1, dh=-1),
            lambda s, m=m, n=n: [X.crop_output(s, (m, 0, 2 * m - 1, 2 * n - 1))])
        add(f"minus1_inner_{kind}", _file(kind, 3, 3, 200 + k, dw=-1, dh=-1), lambda s, m=m, n=n: [X.crop_output(s, (m, n, m, n))])
        add(f"unaligned_size_{kind}", _file(kind, 4, 3, 210 + k), lambda s, m=m, n=n: [X.crop_output(s, (m, n, m + 3, n + 5))])
        # sources with restart markers every 1, 2 and 7 MCUs, cut in the middle of an interval; outputs with every MCU an interval, a row, none
        for r, out_r in ((1, 0), (2, 1), (7, None)):
            add(f"source_dri{r}_{kind}", _file(kind, 5, 3, 220 + 10 * r + k, restart=r),
                lambda s, m=m, n=n, out_r=out_r: [X.crop_output(s, (m, n, 3 * m, 2 * n), restart_mcus=out_r)])
        add(f"swap_dri7_{kind}", _file(kind, 6, 3, 300 + k, restart=7), lambda s: [X.swap_output(s, restart_mcus=4)])
        # optimised tables: a flat image (mid grey: every coefficient zero, so one symbol per table) and noise
        flat = JC.pillow(np.full((2 * n, 4 * m, KINDS[kind][0]), 128, np.uint8), 90, KINDS[kind][1])
        add(f"optimize_flat_{kind}", flat, lambda s: [X.swap_output(s, optimize=True)])
        add(f"optimize_noise_{kind}", _file(kind, 4, 2, 310 + k, noise=True, quality=98), lambda s: X.split_outputs(s, optimize=True, restart_mcus=0))
        add(f"optimize_mixed_{kind}", _file(kind, 4, 2, 320 + k, restart=3),
            lambda s: [X.crop_output(s, optimize=True), X.crop_output(s, (0, 0, s.mw, s.mh))])
    # outputs of 31 ... 33, 255 ... 257 and 511 ... 513 blocks: the gather's workgroup of 32 blocks and the encoder stages' of 256
    for n in (31, 32, 33, 255, 256, 257, 511, 512, 513):
        add(f"blocks_{n}", _file("gray", n + 2, 1, 400 + n, restart=5), lambda s, n=n: [X.crop_output(s, (8, 0, 8 * n, 8))])
    add("blocks_513_444", _file("444", 171, 2, 420, restart=9), lambda s: [X.crop_output(s, (0, 8, 8 * 171, 8), restart_mcus=0)])
    add("blocks_516_422", _file("422", 129, 2, 422, restart=11), lambda s: [X.crop_output(s, (0, 8, 16 * 129, 8), restart_mcus=7)])
    add("blocks_258_420", _file("420", 43, 2, 421), lambda s: [X.crop_output(s, (0, 16, 16 * 43, 16))])
    # a scan that needs more than a handful of synchronisation rounds (the decoder's noise cases), split and swapped
    sup = JC.supported_cases()
    add("noise_q100_420_split", sup["noise_q100_420"], lambda s: X.split_outputs(s))
    add("noise_q100_422_whole", sup["noise_q100_422"], lambda s: [X.crop_output(s, optimize=True), X.crop_output(s, (16, 8, 31, 25))])
    add("dri_blocks_422_swap", JC.pillow(PC.smooth(40, 96, 3, 59), 90, "422", restart_marker_blocks=2), lambda s: [X.swap_output(s)] + X.split_outputs(s))
    add("noise_q100_444_swap", sup["noise_q100_444"], lambda s: [X.swap_output(s)])
    add("noise_q100_gray_crop", sup["noise_q100_gray"], lambda s: [X.crop_output(s, (8, 16, 70, 41), optimize=True)])
    # sources with tables of their own, 16-bit quantisation tables (SOF1), fill bytes, APPn / COM segments (dropped)
    add("optimised_source_420", sup["optimised_420"], lambda s: [X.crop_output(s, (16, 16, 48, 32))])
    add("dqt16_sof1", sup["dqt16_sof1"], lambda s: [X.crop_output(s, (16, 0, 31, 33))])
    add("dqt16_wide", JC.dqt16_values(JC.pillow(PC.smooth(33, 47, 3, 431), 90, "420"), 300), lambda s: [X.crop_output(s, (16, 0, 31, 33))])
    add("fill_bytes_rst", sup["fill_bytes_rst"], lambda s: [X.crop_output(s, (16, 16, 40, 24))])
    add("com_app1", sup["com_app1"], lambda s: [_whole(s)])
    add("one_table_for_all", JC.pillow(PC.smooth(24, 32, 3, 430), 100, "444"), lambda s: [X.swap_output(s)])
    # three and four regions: the quadrants exchanged; two outputs of different sizes
    add("quadrants_420", _file("420", 4, 4, 440, restart=3),
        lambda s: [dict(width=64, height=64, regions=[(2, 2, 2, 2, 0, 0), (0, 2, 2, 2, 2, 0), (2, 0, 2, 2, 0, 2), (0, 0, 2, 2, 2, 2)])])
    add("three_regions_gray", _file("gray", 6, 2, 441),
        lambda s: [dict(width=48, height=16, restart_mcus=0, regions=[(4, 0, 2, 2, 0, 0), (2, 0, 2, 2, 2, 0), (0, 0, 2, 2, 4, 0)])])
    # the largest coefficients the encoder's tables code, next to each other: a DC difference of -2047, AC coefficients of +-1023
    add("coefficient_limits", _coded({(0, 0): 1023, (1, 0): -1024, (0, 5): 1023, (1, 63): -1023, (2, 0): 1023}, 3), 
        lambda s: [dict(width=24, height=8, restart_mcus=0, regions=[(2, 0, 1, 1, 0, 0), (1, 0, 1, 1, 1, 0), (0, 0, 1, 1, 2, 0)])])
    return c


def _coded(values, nblocks, dtype=np.int16, restart=2):
    """a grey file of ``nblocks`` blocks in a row whose coefficients are ``values[(block, zigzag index)]``, zero elsewhere, coded by the
    encoder's restatement with tables built for it: valid syntax whatever the numbers"""
    import jpg_opt_ref as O

    g = R.Geom(8, 8 * nblocks, 1, "420", restart)
    zz = np.zeros((nblocks, 64), dtype)
    for (b, k), v in values.items():
        zz[b, k] = v
    specs = O.tables(zz, g)
    return O.headers(g, 50, specs) + O.scan(zz, g, specs) + b"\xff\xd9"


def excluded_blocks() -> dict:
    """name: (file, outputs): files with a coefficient the encoder's tables do not code in a block that the cut leaves out -- taken: the
    range rule is over the gathered blocks"""
    return {
        "ac_2000_left_out": (_coded({(0, 63): -2000, (1, 0): 5, (2, 7): 3}, 3), [dict(width=16, height=8, regions=[(1, 0, 2, 1, 0, 0)])]),
        "dc_1500_left_out": (_coded({(0, 0): 1500, (1, 0): 900, (2, 0): 100}, 3), [dict(width=16, height=8, regions=[(1, 0, 2, 1, 0, 0)])]),
    }


def out_of_range() -> dict:
    """name: (file, outputs): valid files with a coefficient the encoder's tables do not code, refused after the decode"""
    outs = [dict(width=16, height=8, regions=[(0, 0, 2, 1, 0, 0)])]
    return {
        "dc_1024": (_coded({(0, 0): 1024, (1, 0): 1024}, 2), outs),
        "dc_minus_1025": (_coded({(0, 0): -1025}, 2), outs),
        "dc_1024_in_two_steps": (_coded({(0, 0): 600, (1, 0): 1024}, 2), outs),
        # 34 DC differences of 1930: the sum passes 16 bits and, cut to them, lies inside the range again (65620 - 65536 = 84)
        "dc_sum_wraps_into_range": (_coded({(b, 0): 1930 * (b + 1) for b in range(34)}, 34, np.int32, 34),
                                    [dict(width=8, height=8, regions=[(33, 0, 1, 1, 0, 0)])]),
        "ac_1024": (_coded({(1, 9): 1024}, 2), outs),
        "ac_minus_2000_at_63": (_coded({(0, 63): -2000}, 2), outs),
    }


SLOW_ROUNDS = "noise_q100_420_split"  # the case whose decode takes the most rounds


@functools.lru_cache(maxsize=None)
def reference(name) -> tuple:
    """the restatement's files of a case"""
    data, outputs = cases()[name]
    return tuple(X.transcode(data, outputs))


# ---- what is refused, and with which code ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def refused() -> dict:
    """name: (file, outputs, the exception of jpgxc_ref)"""
    img = PC.smooth(48, 64, 3, 500)
    base = JC.pillow(img, 90, "420")     # 4 x 3 MCUs
    whole = dict(width=64, height=48, regions=[(0, 0, 4, 3, 0, 0)])
    three = JC.pillow(img, 90, "444")
    segs = JC.header_segments(three)
    m, a, e = next(s for s in segs if s[0] == 0xDB)
    # a third quantisation table for Cr: table 2, a copy of table 1 with one entry changed; SOF's Cr names it
    body = three[a + 4:e]
    tables = [body[i:i + 65] for i in range(0, len(body), 65)]
    if len(tables) == 1:  # (Pillow may write one DQT segment per table)
        tables = [three[x + 4:y] for mm, x, y in segs if mm == 0xDB]
    third = bytes([2]) + bytes([tables[1][1] + 1]) + tables[1][2:]
    sm, sa, se = next(s for s in segs if s[0] == 0xC0)
    sof = bytearray(three[sa:se])
    sof[4 + 6 + 3 * 2 + 2] = 2
    three_tables = three[:sa] + JC.segment(0xDB, third) + bytes(sof) + three[se:]
    return {
        "progressive": (JC.pillow(img, 90, "420", progressive=True), [whole], X.Unsupported),
        "sampling_411": (JC.edit_sof(JC.pillow(img, 90, "422"), luma=0x41), [dict(width=64, height=48, regions=[(0, 0, 2, 6, 0, 0)])], X.Unsupported),
        "three_table_classes": (three_tables, [dict(width=64, height=48, regions=[(0, 0, 8, 6, 0, 0)])], X.Unsupported),
        "overlapping_regions": (base, [dict(width=64, height=48, regions=[(0, 0, 3, 3, 0, 0), (0, 0, 2, 3, 2, 0)])], X.Unsupported),
        "uncovered_mcus": (base, [dict(width=64, height=48, regions=[(0, 0, 2, 3, 0, 0), (0, 0, 1, 3, 2, 0)])], X.Invalid),
        "region_outside_source": (base, [dict(width=64, height=48, regions=[(1, 0, 4, 3, 0, 0)])], X.Invalid),
        "region_outside_output": (base, [dict(width=48, height=48, regions=[(0, 0, 4, 3, 0, 0)])], X.Invalid),
        "size_below_the_regions": (base, [dict(width=33, height=32, regions=[(0, 0, 3, 3, 0, 0)])], X.Invalid),
        "no_regions": (base, [dict(width=64, height=48, regions=[])], X.Invalid),
        "seventeen_regions": (base, [dict(width=16 * 17, height=16, regions=[(0, 0, 1, 1, i, 0) for i in range(17)])], X.Invalid),
        "restart_too_large": (base, [dict(whole, restart_mcus=65536)], X.Invalid),
    }


def corrupt() -> dict:
    """name: (file, outputs, whether the parse alone finds it)"""
    out = {}
    for name, (data, by_parse) in JC.corrupt_cases().items():
        try:
            s = D.parse(data)
        except D.Corrupt:  # the parse refuses it: any output will do
            out[name] = (data, [dict(width=8, height=8, regions=[(0, 0, 1, 1, 0, 0)])], True)
            continue
        out[name] = (data, [dict(width=s.w, height=s.h, regions=[(0, 0, s.mcux, s.mcuy, 0, 0)])], by_parse)
    return out
