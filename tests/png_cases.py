"""Images that sit on the boundaries of the device PNG encoder's kernels (csrc/kernels_png.hip), shared by the host half
(tests/test_png_device_host.py) and the GPU half (tests/test_gpu_png_edges.py).  Not a test module.  Seeded and deterministic.

``from_filtered(f)`` builds the gray 8-bit image whose Up-filtered scanline bytes are exactly ``f`` (a cumulative sum down the columns,
modulo 256), so a plane of runs drawn for the scanline bytes themselves can be laid across what only the kernels have: the carry of
the 64-lane steps and the segment start of ``load_segment`` (runs of 62 ... 66, 127 ... 129, 250 ... 257, 300 bytes), a band that is a
whole number of 256-byte segments or ends in a segment of one byte, the 64-segment groups (64 and 65 segments), the 256-wide scan with
its carry (256 and 257 segments), codes with 15-bit lengths and trees that package-merge has to flatten (Fibonacci frequencies), and
the 65 535-byte stored blocks (noise bands of 65 535, 65 536, 65 537, 131 070 and 131 071 bytes).  The same run planes reshaped to BGR,
BGRA and 16-bit images cross ``raw_byte``'s channel and endian swap with those boundaries.
"""
from __future__ import annotations

import numpy as np

import png_ref as R

RUN_LENGTHS = np.array(list(range(1, 7)) + [62, 63, 64, 65, 66, 127, 128, 129, 250, 255, 256, 257, 300])


def from_filtered(f: np.ndarray) -> np.ndarray:
    """(H, W, 1) uint8 image whose Up-filtered scanlines are ``f`` (H, 1 + W); column 0 of ``f`` must hold the filter type 2"""
    f = np.asarray(f, np.uint8)
    assert f.ndim == 2 and (f[:, 0] == 2).all()
    return np.ascontiguousarray((np.cumsum(f[:, 1:].astype(np.int64), axis=0) & 255).astype(np.uint8)[..., None])


def run_bytes(rng, n: int, alphabet: int | None = None) -> np.ndarray:
    """n bytes made of runs of RUN_LENGTHS over an alphabet of 2 ... 6 values, no two neighbouring runs of one value"""
    k = int(rng.integers(2, 7)) if alphabet is None else alphabet
    values = rng.choice(256, k, replace=False)
    lengths = rng.choice(RUN_LENGTHS, n)  # (more than enough: every run is at least one byte)
    lengths = lengths[:int(np.searchsorted(np.cumsum(lengths), n)) + 1]
    step = rng.integers(1, k, lengths.size)  # the next run's value: any other one of the alphabet
    idx = np.cumsum(step) % k
    return np.repeat(values[idx], lengths)[:n].astype(np.uint8)


def run_plane(rng, rows: int, stride: int, alphabet: int | None = None) -> np.ndarray:
    """(rows, stride) scanline bytes: runs laid through the rows one after the other, the filter byte 2 in column 0"""
    f = run_bytes(rng, rows * stride, alphabet).reshape(rows, stride)
    f[:, 0] = 2
    return f


def noise_plane(rng, rows: int, stride: int) -> np.ndarray:
    f = rng.integers(0, 256, (rows, stride), dtype=np.uint8)
    f[:, 0] = 2
    return f


def _fib(n: int) -> list[int]:
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f


def fibonacci_row(rng, symbols: int = 21) -> np.ndarray:
    """one scanline whose byte values have the frequencies 1, 1, 2, 3, 5, ... (the filter byte 2 is the most frequent one) and in which no
    byte repeats its neighbour: every byte is a literal, the unlimited Huffman tree is symbols - 1 deep.  21 symbols: 28 656 bytes."""
    freq = _fib(symbols)[::-1]
    values = [2] + [int(v) for v in rng.choice(np.setdiff1d(np.arange(256), [2]), symbols - 1, replace=False)]
    seq = np.repeat(np.array(values, np.uint8), freq)  # most frequent first: fill the even places, then the odd ones
    n = seq.size
    out = np.empty(n, np.uint8)
    even = (n + 1) // 2
    out[0::2], out[1::2] = seq[:even], seq[even:]
    assert (out[1:] != out[:-1]).all() and out[0] == 2
    return out.reshape(1, n)


def fibonacci_plane(rng, rows: int, stride: int, symbols: int = 24) -> np.ndarray:
    """(rows, stride) scanline bytes drawn with Fibonacci probabilities over ``symbols`` values"""
    p = np.array(_fib(symbols), np.float64)
    values = rng.choice(256, symbols, replace=False)
    f = values[rng.choice(symbols, (rows, stride), p=p / p.sum())].astype(np.uint8)
    f[:, 0] = 2
    return f


def as_channels(gray: np.ndarray, cn: int) -> np.ndarray:
    """the (H, W, 1) plane read as (H, W / cn, cn) pixels"""
    h, w, _ = gray.shape
    assert w % cn == 0
    return np.ascontiguousarray(gray.reshape(h, w // cn, cn))


def cases() -> dict:
    """name -> (image, band_rows); both filters run over all of it"""
    def rng(k):
        return np.random.default_rng([2025, k])

    out = {}
    # a band that is a whole number of segments; one whose last segment holds one byte (1-row bands of 257 bytes)
    out["runs_stride256_8rows"] = (from_filtered(run_plane(rng(1), 24, 256)), 8)
    out["runs_stride257_1row"] = (from_filtered(run_plane(rng(2), 7, 257)), 1)
    # 64 and 65 segments: a full group, and a group of one behind it
    out["runs_16384"] = (from_filtered(run_plane(rng(3), 64, 256)), 64)
    out["runs_16448"] = (from_filtered(run_plane(rng(4), 64, 257)), 64)
    # 256 and 257 segments: the scan's second round takes the carry of the first
    out["runs_65536"] = (from_filtered(run_plane(rng(5), 256, 256)), 256)
    out["runs_65792"] = (from_filtered(run_plane(rng(6), 256, 257)), 256)
    out["runs_65792_two_values"] = (from_filtered(run_plane(rng(7), 300, 257, alphabet=2)), 256)  # (and a shorter second band)
    # Fibonacci frequencies: 15-bit codes, trees deeper than 15
    out["fib21_one_row"] = (from_filtered(fibonacci_row(rng(8), 21)), 1)
    out["fib24_stride602"] = (from_filtered(fibonacci_plane(rng(9), 128, 602, 24)), 64)
    # noise: stored bands around the 65 535-byte block
    out["noise_65535"] = (from_filtered(noise_plane(rng(10), 255, 257)), 255)
    out["noise_65536"] = (from_filtered(noise_plane(rng(11), 256, 256)), 256)
    out["noise_65537"] = (from_filtered(noise_plane(rng(12), 1, 65537)), 1)  # 1 x 65 536 gray
    out["noise_131070"] = (from_filtered(noise_plane(rng(13), 510, 257)), 510)
    out["noise_131071"] = (from_filtered(noise_plane(rng(14), 1, 131071)), 1)
    # a stored band of exactly one block and a coded band in one file
    out["noise_then_runs"] = (from_filtered(np.concatenate([noise_plane(rng(15), 255, 257), run_plane(rng(16), 255, 257)])), 255)
    # the run planes through the channel and endian swap
    out["runs_bgr_stride256"] = (as_channels(out["runs_stride256_8rows"][0], 3), 8)
    out["runs_bgr_16384"] = (as_channels(out["runs_16384"][0], 3), 64)
    out["runs_bgra_stride257_1row"] = (as_channels(out["runs_stride257_1row"][0], 4), 1)
    out["runs_bgra_65792"] = (as_channels(out["runs_65792"][0], 4), 256)
    out["runs_gray16_stride257"] = (R._wide16(from_filtered(run_plane(rng(17), 9, 129))), 1)
    out["runs_gray16_16448"] = (R._wide16(from_filtered(run_plane(rng(18), 64, 129))), 64)
    out["runs_bgr16_stride769"] = (R._wide16(as_channels(from_filtered(run_plane(rng(19), 86, 385)), 3)), 43)
    out["runs_bgra16_65792"] = (R._wide16(as_channels(from_filtered(run_plane(rng(20), 256, 129)), 4)), 256)
    return out


def random_image(rng):
    """(description, image, band_rows) for the fuzz: one of the generators above with random parameters and a random band height"""
    kind = int(rng.integers(0, 5))
    rows = int(rng.integers(1, 200))
    stride = int(rng.choice([2, 5, 64, 65, 255, 256, 257, 258, 512, 513, 602, 769, int(rng.integers(2, 1400))]))
    if kind == 0:
        f, name = run_plane(rng, rows, stride), "runs"
    elif kind == 1:
        f, name = noise_plane(rng, rows, stride), "noise"
    elif kind == 2:
        f, name = fibonacci_plane(rng, rows, stride, int(rng.integers(16, 40))), "fibonacci"
    elif kind == 3:
        top = int(rng.integers(0, rows + 1))
        f, name = np.concatenate([noise_plane(rng, top, stride), run_plane(rng, rows - top, stride)]), f"noise{top}+runs"
    else:
        f, name = fibonacci_row(rng, int(rng.integers(16, 24))), "fibonacci-row"
        rows, stride = f.shape
    img = from_filtered(f)
    w = img.shape[1]
    form = "gray"
    pick = rng.random()
    if pick < 0.25 and w % 3 == 0:
        img, form = as_channels(img, 3), "bgr"
    elif pick < 0.5 and w % 4 == 0:
        img, form = as_channels(img, 4), "bgra"
    if rng.random() < 0.3:
        img, form = R._wide16(img), form + "16"
    band_rows = int(rng.choice([1, 2, 8, rows, int(rng.integers(1, rows + 1)), max(1, 65536 // stride), max(1, 65535 // stride + 1)]))
    return f"{name} {form} {img.shape[1]}x{img.shape[0]} stride={1 + img.shape[1] * img.shape[2] * img.dtype.itemsize} band_rows={band_rows}", img, band_rows


def band_stats(img: np.ndarray, filter: str, band_rows: int) -> list[dict]:
    """per band of the restated stream: stored?, the longest code length, the depth of the unlimited Huffman tree, the match lengths"""
    lines = R.scanlines(img, filter)
    h = lines.shape[0]
    rows = min(band_rows, h)
    out = []
    for r in range(0, h, rows):
        s = lines[r:r + rows].reshape(-1)
        pos, kind, length = R.tokens(s)
        sym = np.where(kind == 1, s[pos].astype(np.int64), R.LEN_SYM[length])
        freq = np.bincount(sym, minlength=286)
        freq[256] = 1
        out.append({"stored": R.band(s)[1], "max_len": int(R.code_lengths(freq, 15).max()), "depth": int(R.code_lengths(freq, 300).max()),
                    "matches": set(int(v) for v in length[kind == 2]), "nbytes": int(s.size)})
    return out


_CASES: dict = {}
_REFERENCE: dict = {}


def shared_cases() -> dict:
    """``cases()``, built once per process"""
    if not _CASES:
        _CASES.update(cases())
    return _CASES


def reference(name: str, filter: str):
    """(segments, bands, file) of the restatement for one case and filter, computed once per process and shared by the tests"""
    key = (name, filter)
    if key not in _REFERENCE:
        img, rows = shared_cases()[name]
        segs, bands = R.deflate(img, filter=filter, band_rows=rows)
        _REFERENCE[key] = (segs, bands, R.encode(img, filter=filter, band_rows=rows))
    return _REFERENCE[key]
