"""The boundary files of the device JPEG decoder, shared by the host half (tests/test_jpegdec_host.py: the restatement against
itself and Pillow, the product's arithmetic on the CPU against the restatement, and the proof that the list holds what it is for) and
the GPU half (tests/test_gpu_jpegdec_edges.py: the kernels against the same values).  Files are written by Pillow (every sampling,
optimised tables, its restart options), by the encoder's restatement (jpg_ref.encode: any restart interval) or edited byte-wise.
Every case is a fraction of a second; the restatement of each is computed once and shared."""
from __future__ import annotations

import functools
import io
import struct

import numpy as np

import jpg_cases as PC
import jpg_ref as R
import jpgdec_ref as D

SAMPLINGS = {"444": 0, "422": 1, "420": 2}  # Pillow's numbering
NOISE_SEED = 1


def pillow(img, quality=95, sampling="420", **kw) -> bytes:
    """a file of a BGR (h, w, 3) or grey (h, w) image by Pillow: no restart markers unless asked for"""
    from PIL import Image

    b = io.BytesIO()
    if img.ndim == 2 or img.shape[2] == 1:
        Image.fromarray(np.ascontiguousarray(img.reshape(img.shape[:2]))).save(b, "JPEG", quality=quality, **kw)
    else:
        Image.fromarray(np.ascontiguousarray(img[..., ::-1])).save(b, "JPEG", quality=quality, subsampling=SAMPLINGS[sampling], **kw)
    return b.getvalue()


# ---- byte-wise edits ------------------------------------------------------------------------------------------------------------------
def header_segments(data):
    """[(marker, first byte of 0xFF, byte behind the segment)] up to and including SOS"""
    out, pos = [], 2
    while True:
        assert data[pos] == 0xFF
        m = data[pos + 1]
        end = pos + 2 + struct.unpack(">H", data[pos + 2:pos + 4])[0]
        out.append((m, pos, end))
        if m == 0xDA:
            return out
        pos = end


def segment(marker, body):
    return struct.pack(">BBH", 0xFF, marker, len(body) + 2) + body


def without(data, marker):
    for m, a, e in reversed(header_segments(data)):
        if m == marker:
            data = data[:a] + data[e:]
    return data


def insert_after_soi(data, *segs):
    return data[:2] + b"".join(segs) + data[2:]


def dqt16_sof1(data):
    """every DQT table rewritten with 16-bit entries, SOF0 turned into SOF1"""
    out = data
    for m, a, e in reversed(header_segments(data)):
        if m == 0xDB:
            body, new, i = data[a + 4:e], b"", 0
            while i < len(body):
                assert body[i] >> 4 == 0
                new += bytes([0x10 | body[i]]) + b"".join(struct.pack(">H", v) for v in body[i + 1:i + 65])
                i += 65
            out = out[:a] + segment(0xDB, new) + out[e:]
        elif m == 0xC0:
            out = out[:a + 1] + b"\xc1" + out[a + 2:]
    return out


def fill_bytes(data):
    """0xFF fill bytes in front of every header marker behind SOI, of the first RSTm if there is one, and of EOI"""
    segs = header_segments(data)
    scan = data[segs[-1][2]:-2]
    i = next((i for i in range(len(scan) - 1) if scan[i] == 0xFF and 0xD0 <= scan[i + 1] <= 0xD7), None)
    if i is not None:
        scan = scan[:i] + b"\xff\xff" + scan[i:]
    head = data[:2] + b"".join(b"\xff" * (1 + k % 3) + data[a:e] for k, (m, a, e) in enumerate(segs))
    return head + scan + b"\xff\xff\xff" + data[-2:]


def merged_dht(data):
    """all DHT tables in one segment, where the first one was"""
    segs = header_segments(data)
    bodies = b"".join(data[a + 4:e] for m, a, e in segs if m == 0xC4)
    at = next(a for m, a, e in segs if m == 0xC4)
    rest = without(data, 0xC4)  # (what lies in front of the first one does not move)
    return rest[:at] + segment(0xC4, bodies) + rest[at:]


def edit_sof(data, **kw):
    """SOF fields rewritten: width=, luma= (the sampling byte of the first component)"""
    m, a, e = next(s for s in header_segments(data) if s[0] in (0xC0, 0xC1))
    b = bytearray(data)
    if "width" in kw:
        b[a + 7:a + 9] = struct.pack(">H", kw["width"])
    if "luma" in kw:
        b[a + 11] = kw["luma"]
    return bytes(b)


def edit_dri(data, value):
    m, a, e = next(s for s in header_segments(data) if s[0] == 0xDD)
    return data[:a + 4] + struct.pack(">H", value) + data[e:]


def edit_dht(data, tc_th, counts):
    """the 16 code counts of table ``tc_th`` (0x00 DC 0, 0x10 AC 0, ...) rewritten; ``counts`` must keep their sum, so that the
    segment stays well-formed and only the table is wrong"""
    b = bytearray(data)
    for m, a, e in header_segments(data):
        i = a + 4
        while m == 0xC4 and i < e:
            n = sum(b[i + 1:i + 17])
            if b[i] == tc_th:
                assert sum(counts) == n and len(counts) == 16
                b[i + 1:i + 17] = bytes(counts)
                return bytes(b)
            i += 17 + n
    raise KeyError(tc_th)


def dqt16_values(data, value):
    """``dqt16_sof1`` with every entry set to ``value``"""
    out = dqt16_sof1(data)
    for m, a, e in reversed(header_segments(out)):
        if m == 0xDB:
            body, new, i = out[a + 4:e], b"", 0
            while i < len(body):
                new += bytes([body[i]]) + struct.pack(">H", value) * 64
                i += 129
            out = out[:a] + segment(0xDB, new) + out[e:]
    return out


ADOBE_RGB = segment(0xEE, b"Adobe\x00\x64\x00\x00\x00\x00\x00")  # version 100, flags 0, transform 0


# ---- the list -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def supported_cases() -> dict:
    c = {}
    for i, (h, w) in enumerate(PC.SIZES):
        for s in SAMPLINGS:
            c[f"size_{h}x{w}_{s}"] = pillow(PC.smooth(h, w, 3, 10 + i), 95, s)
        c[f"size_{h}x{w}_gray"] = pillow(PC.smooth(h, w, 1, 30 + i), 95)
    # restart intervals: none above; 1; one that ends mid-row; the MCU count; more; 65535; 45 intervals (RSTm wraps five times)
    c["dri1_444"] = R.encode(PC.smooth(40, 72, 3, 52), 95, "444", 1)
    c["dri1_gray"] = R.encode(PC.smooth(24, 40, 1, 57), 95, "420", 1)
    c["midrow_420_r3"] = R.encode(PC.smooth(40, 72, 3, 50), 95, "420", 3)
    c["midrow_444_r7"] = R.encode(PC.smooth(40, 72, 3, 51), 95, "444", 7)
    c["dri_exact"] = R.encode(PC.smooth(40, 72, 3, 54), 95, "420", 15)
    c["dri_more"] = R.encode(PC.smooth(40, 72, 3, 55), 95, "420", 16)
    c["dri_65535"] = R.encode(PC.smooth(24, 24, 1, 56), 95, "420", 65535)
    c["dri_rows_422"] = pillow(PC.smooth(40, 72, 3, 58), 95, "422", restart_marker_rows=1)
    c["dri_blocks_422"] = pillow(PC.smooth(40, 72, 3, 59), 90, "422", restart_marker_blocks=2)
    c["dri2_420_noise"] = R.encode(PC.noise(48, 64, 3, 62), 100, "420", 2)
    # sync boundaries
    c["flat_420"] = pillow(np.full((128, 160, 3), 128, np.uint8), 95, "420")               # EOB-only blocks, a few bits each
    c["flat_gray_200"] = pillow(np.full((64, 200), 200, np.uint8), 50)
    c["only_63"] = without(R.encode(PC.from_coefficients([{63: 2}, {63: -1}, {0: 3, 63: 1}], 50), 50, restart_mcus=3), 0xDD)
    c["zero_runs"] = without(R.encode(PC.from_coefficients([{16: 1, 33: -1, 51: 1}, {34: 1}, {17: -1, 35: 1}, {0: -2, 1: 1, 63: 1}], 50), 50,
                                      restart_mcus=4), 0xDD)
    c["swing_q100"] = without(R.encode(PC.swing(), 100, restart_mcus=8), 0xDD)
    c["noise_q100_444"] = pillow(PC.noise(64, 96, 3, NOISE_SEED), 100, "444")
    c["noise_q100_420"] = pillow(PC.noise(64, 96, 3, NOISE_SEED + 1), 100, "420")
    c["noise_q100_422"] = pillow(PC.noise(33, 47, 3, NOISE_SEED + 2), 100, "422")
    c["noise_q100_gray"] = pillow(PC.noise(64, 96, 1, NOISE_SEED + 3), 100)
    c["optimised_420"] = pillow(PC.noise(48, 80, 3, 63) // 2 + PC.smooth(48, 80, 3, 64) // 2, 90, "420", optimize=True)
    c["optimised_444_smooth"] = pillow(PC.smooth(40, 72, 3, 65), 75, "444", optimize=True)
    c["optimised_gray"] = pillow(PC.noise(40, 56, 1, 66), 95, optimize=True)
    c["quality_1"] = pillow(PC.smooth(33, 47, 3, 71), 1, "420")
    c["quality_100"] = pillow(PC.smooth(33, 47, 3, 72), 100, "420")
    # byte-edited files
    base = pillow(PC.smooth(33, 47, 3, 73), 90, "420")
    c["dqt16_sof1"] = dqt16_sof1(base)
    c["com_app1"] = insert_after_soi(base, segment(0xFE, b"a comment"), segment(0xE1, b"Exif\x00\x00" + bytes(40)))
    c["fill_bytes"] = fill_bytes(base)
    c["fill_bytes_rst"] = fill_bytes(c["midrow_420_r3"])
    c["merged_dht"] = merged_dht(base)
    c["junk_after_eoi"] = base + b"\x00\xff\xd8junk\xff\xd9\xff"
    c["adobe_ycc"] = insert_after_soi(without(base, 0xE0), segment(0xEE, b"Adobe\x00\x64\x00\x00\x00\x00\x01"))
    return c


@functools.lru_cache(maxsize=None)
def extreme_cases() -> dict:
    """valid syntax, absurd numbers: 16-bit quantiser entries times large coefficients, which the contract saturates to 16 bits in
    front of the inverse DCT.  Held to the restatement like the supported cases; Pillow is no yardstick here."""
    return {
        "dqt16_60000_swing": dqt16_values(without(R.encode(PC.swing(), 100, restart_mcus=8), 0xDD), 60000),
        "dqt16_4000_noise_420": dqt16_values(pillow(PC.noise(24, 40, 3, 69), 100, "420"), 4000),
    }


@functools.lru_cache(maxsize=None)
def unsupported_cases() -> dict:
    img = PC.smooth(33, 47, 3, 74)
    base = pillow(img, 90, "420")
    return {
        "progressive": pillow(img, 90, "420", progressive=True),
        "sampling_411": edit_sof(pillow(img, 90, "422"), luma=0x41),
        "sampling_440": edit_sof(pillow(img, 90, "422"), luma=0x12),
        "adobe_transform_0": insert_after_soi(without(pillow(img, 90, "444"), 0xE0), ADOBE_RGB),
        "two_scans": base[:-2] + base[header_segments(base)[-1][1]:],
    }


@functools.lru_cache(maxsize=None)
def corrupt_cases() -> dict:
    """name: (file, whether the parse alone finds it)"""
    noise = pillow(PC.noise(24, 40, 1, 67), 95)
    dri = R.encode(PC.smooth(40, 72, 3, 50), 95, "420", 3)
    first = dri.index(b"\xff\xd0")
    few = edit_dri(edit_sof(R.encode(PC.smooth(8, 32, 1, 68), 95, "420", 2), width=40), 3)
    base = pillow(PC.smooth(33, 47, 3, 73), 90, "420")
    n_dc, n_ac = 12, 162  # symbols of the Annex K tables Pillow writes
    return {
        # DHT tables that declare more codes of a length than the length holds: short lengths (inside the decoder's lookup), DC and AC
        "dht_dc_3_codes_of_1_bit": (edit_dht(base, 0x00, [3, 0, n_dc - 3] + [0] * 13), True),
        "dht_ac_all_codes_of_1_bit": (edit_dht(base, 0x10, [n_ac] + [0] * 15), True),
        "dht_ac_5_codes_of_2_bits": (edit_dht(base, 0x11, [0, 5, 0, 0, 0, 0, 0, 0, n_ac - 5] + [0] * 7), True),
        "dht_dc_long_length_overfull": (edit_dht(base, 0x01, [2, 0, 0, 0, 0, 0, 0, 0, 0, n_dc - 2] + [0] * 6), True),
        "dht_alone_255_codes_of_1_bit": (b"\xff\xd8" + segment(0xC4, bytes([0x00, 255] + [0] * 15) + bytes(255)), True),
        "truncated": (noise[:-5] + noise[-2:], False),
        "no_eoi": (noise[:-2], True),
        "rst1_for_rst0": (dri[:first + 1] + b"\xd1" + dri[first + 2:], True),
        "one_block_too_few": (few, False),
    }


TRUNCATED = "truncated"  # the corrupt case that also runs on the device


@functools.lru_cache(maxsize=None)
def reference(name, S=0):
    """the restatement of a supported or extreme case"""
    data = supported_cases().get(name) or extreme_cases()[name]
    return D.decode(data, S)
