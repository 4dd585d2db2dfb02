"""Float64 statement of what a baseline JPEG encoder's quantised coefficients have to be: BGR -> YCbCr by the JFIF definition -> 2 x 2
mean (4:2:0) -> level shift -> orthonormal 8 x 8 DCT-II -> division by the quantisation table.

Not a test module: tests/test_jpeg_analytic_host.py holds the NumPy restatement (jpg_ref.py) and the host build of jpeg_core.hpp to it
on the CPU, tests/test_gpu_jpeg_analytic.py the files the MI355X writes.  From jpg_ref.py it takes only what the standard fixes --
ZIGZAG, the Annex K tables and the IJG quality rule, themselves held to Pillow's ``im.quantization`` -- and a file's coefficients are
read back by jpgdec_ref.py, the decoder's restatement that is held to Pillow pixel for pixel: the encoder's restatement is not on the
path.  Every sum runs in float64.

Samples are intervals.  JPEG's DCT input is 8-bit samples, and at a rounding tie the direction is the implementation's choice, so every
sample is [lo, hi] (midpoint and half-width): lo = hi where the rounding is forced; [k, k + 1] where the float64 conversion lies within
EPS_C of k + 0.5; for 4:2:0 chroma the sums of the four [lo, hi] of the cell, rounded to nearest with a sum = 2 (mod 4) going either
way (the contract rounds half up, libjpeg alternates).

The hold:  |c q - F| <= q / 2 + delta[v, u] + sum_xy |C[v, y] C[u, x]| halfwidth(y, x)  for every coefficient c of every block, with F
the DCT of (midpoint - 128).  q / 2 is the quantiser's rounding, the last term what the samples' intervals can move F by, and delta the
error bound of the IJG "islow" integer DCT derived below.
"""
from __future__ import annotations

import numpy as np

import jpgdec_ref as D
from jpg_ref import Q_CHROMA, Q_LUMA, ZIGZAG, quant_table

# ----------------------------------------------------------------------------------------------------------------------- colour
# EPS_C: how far a 16-bit fixed-point colour conversion can lie from the float64 one.  A plane is a sum of three products of an 8-bit
# value (<= 255) with a constant held in 16 fractional bits (<= 2^-17 off when rounded to nearest), so 3 * 255 * 2^-17 = 0.00584; libjpeg
# adds ONE_HALF - 1 in place of ONE_HALF for the chroma planes, 2^-16 more.  (libjpeg's -0.16874 and -0.33126 are five-digit values
# and lie 0.73 units of 2^-16 off the JFIF ones, but the third term of that plane, 0.5 B, is exact: tests/test_jpeg_analytic_host.py
# checks that the contract's constants stay inside EPS_C.)
EPS_C = 3 * 255 * 2.0 ** -17 + 2.0 ** -16
FLOAT_SLACK = 1e-9  # float64 rounding of F (|F| <= 1024, 128 terms): orders of magnitude below this


def ycc(img: np.ndarray) -> list[np.ndarray]:
    """float64 planes of an (h, w, cn) uint8 image in cv2 channel order: [grey] or [Y, Cb, Cr] (JFIF); alpha is dropped"""
    a = img.astype(np.float64)
    if a.shape[2] == 1:
        return [a[..., 0]]
    b, g, r = a[..., 0], a[..., 1], a[..., 2]
    y = 0.299 * r + 0.587 * g + 0.114 * b
    return [y, (b - y) / 1.772 + 128.0, (r - y) / 1.402 + 128.0]


def mcu_edge(cn: int, subsampling: str) -> int:
    return 16 if (cn != 1 and subsampling == "420") else 8


def sample_intervals(img: np.ndarray, subsampling: str = "420"):
    """[(lo, hi), ...] per component: int64 planes padded to whole MCUs by repeating the last column and row (before downsampling)"""
    a = img if img.ndim == 3 else img[..., None]
    h, w, cn = a.shape
    assert cn in (1, 3, 4) and subsampling in ("420", "444")
    m = mcu_edge(cn, subsampling)
    a = np.pad(a, ((0, -h % m), (0, -w % m), (0, 0)), mode="edge")
    if cn == 1:
        p = a[..., 0].astype(np.int64)
        return [(p, p)]
    out = []
    for k, v in enumerate(ycc(a)):
        lo = np.clip(np.ceil(v - 0.5 - EPS_C), 0, 255).astype(np.int64)  # (an 8-bit sample: Cb of pure blue is 255.5 and is held as 255)
        hi = np.clip(np.floor(v + 0.5 + EPS_C), 0, 255).astype(np.int64)
        if k and m == 16:
            slo, shi = [p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] for p in (lo, hi)]
            lo, hi = (slo + 1) // 4, (shi + 2) // 4  # s / 4 to nearest; s = 2 (mod 4) down in lo, up in hi
        out.append((lo, hi))
    return out


def _mcu_blocks(p: np.ndarray, n: int) -> np.ndarray:
    """(mcuy, mcux, n * n, 8, 8): the n x n blocks of every MCU of a plane, in raster order inside the MCU"""
    my, mx = p.shape[0] // (8 * n), p.shape[1] // (8 * n)
    return p.reshape(my, n, 8, mx, n, 8).transpose(0, 3, 1, 4, 2, 5).reshape(my, mx, n * n, 8, 8)


def sample_blocks(img: np.ndarray, subsampling: str = "420"):
    """(mid, halfwidth, comp): (nblocks, 8, 8) float64 samples in scan order -- MCU by MCU, its Y block(s), Cb, Cr -- and the component
    of every block"""
    a = img if img.ndim == 3 else img[..., None]
    iv = sample_intervals(a, subsampling)
    n = 2 if mcu_edge(a.shape[2], subsampling) == 16 else 1
    los = np.concatenate([_mcu_blocks(iv[0][0], n)] + [_mcu_blocks(lo, 1) for lo, _ in iv[1:]], axis=2)
    his = np.concatenate([_mcu_blocks(iv[0][1], n)] + [_mcu_blocks(hi, 1) for _, hi in iv[1:]], axis=2)
    comp = np.tile(np.array([0] * (n * n) + list(range(1, len(iv)))), los.shape[0] * los.shape[1])
    los, his = los.reshape(-1, 8, 8).astype(np.float64), his.reshape(-1, 8, 8).astype(np.float64)
    return (los + his) / 2, (his - los) / 2, comp


# ----------------------------------------------------------------------------------------------------------------------- transform
def basis() -> np.ndarray:
    """C[u, x] of the orthonormal DCT-II on eight points (as jpg_cases._basis states it)"""
    k = np.arange(8)
    return np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16) * np.where(k[:, None] == 0, np.sqrt(0.5), 1.0) / 2


def dct(blocks: np.ndarray) -> np.ndarray:
    """(n, 8, 8) -> F[n, v, u] = sum_yx C[v, y] C[u, x] s[n, y, x]"""
    c = basis()
    return c @ blocks @ c.T


# delta: the error bound of the IJG "islow" forward DCT (jfdctint.c, Loeffler-Ligtenberg-Moschytz), in coefficient units, derived from
# its rounding steps -- not fitted to any implementation.  The transform runs one 1-D pass over the rows and one over the columns.  A
# pass is the linear map M = G + E, G = 2 sqrt(2) C the exact one and E what rounding the twelve constants to 13 bits does to it (rows
# 0 and 4 are sums and differences only: E = 0 there).  Pass 1 gives 4 M x, descaled by 11 bits except in columns 0 and 4, which are
# exact (a shift left); pass 2 gives M x / 4, descaled by 15 bits, rows 0 and 4 by 2 bits.  So, in output units (8 per coefficient unit),
#   out = (M X M^T)[v, u] + (1 / 4) sum_y M[v, y] e1[y, u] + e2[v, u],   X = samples - 128, |X| <= 128
#   constants:        |M X M^T - G X G^T| = |E X G^T + G X E^T + E X E^T| <= 128 (sE[v] sG[u] + sG[v] sE[u] + sE[v] sE[u]), s = row sum of | |
#   pass-1 descale:   |e1| <= 1 / 2 (0 for u in {0, 4}), and its gain through pass 2 and the division by 4 is sum_y |M[v, y]| / 4 (<= 2, at v = 0)
#   pass-2 descale:   |e2| <= 1 / 2; 0 where v and u are both in {0, 4}: the inputs are multiples of 4 and only added
# and delta[v, u] is their sum over 8.  delta[0, 0] = 0: the DC is exact.  The largest entry is 0.314 at (3, 3) (DELTA below): 0.176 of
# rounding and 0.138 of constants; rounding alone is largest in row 0, 1.5 / 8 = 0.1875.  _flow states the LLM graph once, so that the real constants can be shown to give G exactly
# (``islow_matrices`` asserts it) and the 13-bit ones give E.
_C = [np.cos(k * np.pi / 16) for k in range(8)]
_R2 = np.sqrt(2.0)
ISLOW_REAL = {  # the twelve multipliers by jfdctint.c's names, from their trigonometric definitions
    "0_298631336": _R2 * (-_C[1] + _C[3] + _C[5] - _C[7]), "0_390180644": _R2 * (_C[3] - _C[5]), "0_541196100": _R2 * _C[6],
    "0_765366865": _R2 * (_C[2] - _C[6]), "0_899976223": _R2 * (_C[3] - _C[7]), "1_175875602": _R2 * _C[3],
    "1_501321110": _R2 * (_C[1] + _C[3] - _C[5] - _C[7]), "1_847759065": _R2 * (_C[2] + _C[6]), "1_961570560": _R2 * (_C[3] + _C[5]),
    "2_053119869": _R2 * (_C[1] + _C[3] - _C[5] + _C[7]), "2_562915447": _R2 * (_C[1] + _C[3]),
    "3_072711026": _R2 * (_C[1] + _C[3] + _C[5] - _C[7]),
}
CONST_BITS = 13
ISLOW_13BIT = {k: float(np.rint(v * (1 << CONST_BITS))) / (1 << CONST_BITS) for k, v in ISLOW_REAL.items()}


def _flow(d: np.ndarray, k: dict) -> np.ndarray:
    """the islow flow graph along axis 0 with the multipliers ``k``, in float64 and without any rounding: a linear map"""
    t0, t7, t1, t6, t2, t5, t3, t4 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6], d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    out = [None] * 8
    out[0], out[4] = t10 + t11, t10 - t11
    z1 = (t12 + t13) * k["0_541196100"]
    out[2], out[6] = z1 + t13 * k["0_765366865"], z1 - t12 * k["1_847759065"]
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * k["1_175875602"]
    t4, t5, t6, t7 = t4 * k["0_298631336"], t5 * k["2_053119869"], t6 * k["3_072711026"], t7 * k["1_501321110"]
    z1, z2, z3, z4 = -z1 * k["0_899976223"], -z2 * k["2_562915447"], -z3 * k["1_961570560"] + z5, -z4 * k["0_390180644"] + z5
    out[7], out[5], out[3], out[1] = t4 + z1 + z3, t5 + z2 + z4, t6 + z2 + z3, t7 + z1 + z4
    return np.stack(out)


def islow_matrices():
    """(G, M): the exact pass 2 sqrt(2) C and the pass with the 13-bit constants"""
    g = 2 * _R2 * basis()
    assert np.abs(_flow(np.eye(8), ISLOW_REAL) - g).max() < 1e-12  # the graph with real multipliers IS the DCT
    return g, _flow(np.eye(8), ISLOW_13BIT)


def _delta_table() -> np.ndarray:
    g, m = islow_matrices()
    se, sg, sm = np.abs(m - g).sum(1), np.abs(g).sum(1), np.abs(m).sum(1)
    exact = np.isin(np.arange(8), (0, 4))
    assert np.all(se[exact] < 1e-14)
    se = np.where(exact, 0.0, se)
    constants = 128.0 * (se[:, None] * sg[None, :] + sg[:, None] * se[None, :] + se[:, None] * se[None, :])
    pass1 = 0.25 * sm[:, None] * np.where(exact, 0.0, 0.5)[None, :]
    pass2 = np.where(exact[:, None] & exact[None, :], 0.0, 0.5)
    return (constants + pass1 + pass2) / 8.0


DELTA_TABLE = _delta_table()          # [v, u]
DELTA = float(DELTA_TABLE.max())      # the scalar bound; at q = 1 anything >= 0.5 would let a coefficient be off by a whole level
DELTA_ROUNDING = 1.5 / 8              # its share that is rounding alone, at v = 0: what no derivation can go below
assert DELTA_ROUNDING < DELTA < 0.5


def constants_term(x: np.ndarray) -> np.ndarray:
    """(M X M^T - G X G^T) / 8 of level-shifted blocks: what the 13-bit constants move every coefficient by, exactly -- linear in the
    samples, so its mean over an image is known and enters the bias limits"""
    g, m = islow_matrices()
    return (m @ x @ m.T - g @ x @ g.T) / 8.0


# ----------------------------------------------------------------------------------------------------------------------- the hold
def tables_for(quality: int, ncomp: int) -> list[np.ndarray]:
    """the row-major table of every component at a quality (IJG rule on Annex K)"""
    return [quant_table(Q_LUMA, quality)] + [quant_table(Q_CHROMA, quality)] * (ncomp - 1)


def file_coefficients(data: bytes):
    """(coefficients (nblocks, 64) in zigzag order with the DC a value, info) of a file, by the decoder's restatement"""
    r = D.decode(data, check=False)
    return D.dc_values(r.info, r.coef).astype(np.int64), r.info


# Bias, at quality 100 (every q = 1, so c - F is a rounding error), over the coefficients with |F| >= 1:
#   plain  = mean(c - F),   signed = mean(sign(F) (c - F)).
# The quantiser divides an integer (the DCT output times 8) by 8: of the residues 0 ... 7 only 4 is a tie, and rounding it away from
# zero gives +-4 / 8 one time in eight, so signed = +1 / 16 and plain = (p+ - p-) / 16 with p+-, the shares of positive and negative F.
# Around those: (a) the islow mean error -- descale(x, 2) rounds quarter steps half up, mean +1 / 8 of an output unit = 1 / 64
# (rows 0 and 4; the 11- and 15-bit descales have means 2^-12 and 2^-16 of an output unit) -- plus the mean of ``constants_term``, which is
# computed, not bounded; (b) 5 sigma / sqrt(n) with sigma = 1 / sqrt(12), the uniform rounding error's.  A truncating quantiser has
# signed near -7 / 16, one that rounds half up has plain near +1 / 16 whatever the signs.  n >= BIAS_MIN_N keeps (b) below 1 / 32, so that
# (a) + (b) < 1 / 16 and both of those fall outside.
TIE_BIAS = 1.0 / 16
ISLOW_MEAN = 1.0 / 64
BIAS_MIN_N = 4096
assert ISLOW_MEAN + 5 / np.sqrt(12 * BIAS_MIN_N) < TIE_BIAS


def hold(coef_zz: np.ndarray, tables: list[np.ndarray], img: np.ndarray, subsampling: str = "420") -> dict:
    """Hold quantised coefficients ((nblocks, 64), zigzag order, scan order) to the float64 statement.  Returns the figures and asserts
    nothing: 'excess' = max(|c q - F| - bound) (<= 0 passes), 'max' = the largest |c q - F| - q / 2 - the interval term (what delta has to
    cover), 'n', 'bad', 'ambiguous' = samples of half-width > 0; with every q = 1 and no ambiguous sample also 'plain', 'signed', their
    expected values and limits and 'bias_n'."""
    a = img if img.ndim == 3 else img[..., None]
    mid, hw, comp = sample_blocks(a, subsampling)
    assert coef_zz.shape == (len(mid), 64), (coef_zz.shape, mid.shape)
    x = mid - 128.0
    f = dct(x)
    ca = np.abs(basis())
    width = ca @ hw @ ca.T
    q = np.stack([np.asarray(t).reshape(8, 8) for t in tables]).astype(np.float64)[comp]
    c = np.zeros((len(mid), 64), np.float64)
    c[:, ZIGZAG] = coef_zz
    c = c.reshape(-1, 8, 8)
    dev = np.abs(c * q - f)
    ex = dev - (q / 2 + DELTA_TABLE[None] + width + FLOAT_SLACK)
    out = {"excess": float(ex.max()), "max": float((dev - q / 2 - width).max()), "n": int(ex.size), "bad": int((ex > 0).sum()),
           "ambiguous": int((hw > 0).sum())}
    if np.all(q == 1) and not (hw > 0).any():
        sel = np.abs(f) >= 1.0
        e = (c - f)[sel]
        n = int(sel.sum())
        sign = np.sign(f[sel])
        t = constants_term(x)[sel]
        stat = 5.0 / np.sqrt(12.0 * max(n, 1))
        out.update({"bias_n": n, "plain": float(e.mean()) if n else 0.0, "signed": float((sign * e).mean()) if n else 0.0,
                    "plain_expected": float(sign.mean() * TIE_BIAS) if n else 0.0, "signed_expected": TIE_BIAS,
                    "plain_limit": ISLOW_MEAN + abs(float(t.mean())) + stat if n else 0.0,
                    "signed_limit": ISLOW_MEAN + abs(float((sign * t).mean())) + stat if n else 0.0})
    return out


def bias_ok(f: dict) -> bool:
    """the bias pair of a quality-100 ``hold`` of an image without ambiguous samples"""
    return (f["bias_n"] >= BIAS_MIN_N and abs(f["plain"] - f["plain_expected"]) <= f["plain_limit"]
            and abs(f["signed"] - f["signed_expected"]) <= f["signed_limit"])


def hold_file(data: bytes, img: np.ndarray, quality: int, subsampling: str = "420") -> dict:
    """``hold`` for a file: its frame header must describe the image, its tables must be the quality's"""
    a = img if img.ndim == 3 else img[..., None]
    coef, s = file_coefficients(data)
    nc = 1 if a.shape[2] == 1 else 3
    assert (s.h, s.w, s.nc) == (a.shape[0], a.shape[1], nc), (s.h, s.w, s.nc, a.shape)
    assert (s.hs, s.vs) == ((2, 2) if mcu_edge(a.shape[2], subsampling) == 16 else (1, 1)), (s.hs, s.vs)
    want = tables_for(quality, nc)
    tabs = [s.q[s.tq[k]] for k in range(nc)]
    assert all(np.array_equal(t, w) for t, w in zip(tabs, want)), "the file's tables are not the quality's"
    return hold(coef, tabs, a, subsampling)


def describe(label: str, f: dict) -> str:
    s = f"jpeg analytic {label}: excess {f['excess']:+.4f} max {f['max']:.4f} n {f['n']} ambiguous {f['ambiguous']}"
    if "bias_n" in f:
        s += (f" | plain {f['plain']:+.4f} (expected {f['plain_expected']:+.4f} +- {f['plain_limit']:.4f}) signed {f['signed']:+.4f}"
              f" (expected {f['signed_expected']:+.4f} +- {f['signed_limit']:.4f}) n {f['bias_n']}")
    return s


# ----------------------------------------------------------------------------------------------------------------------- the constants
# What the hold cannot see.  One unit of a 13-bit constant is twice the rounding the honest constants already carry, and it moves a
# coefficient by 0.125 per pass at full swing (a multiplicand of 1024 over 2048 in pass 1, through the gain 2 of pass 2, over 8), by
# far less on ordinary blocks -- less than the rounding delta has to allow (up to 0.1875).  So a wrong constant is caught by the hold only
# where a full-swing block happens to sit at a rounding tie.  The constants are therefore estimated: at q = 1 on a grey image (exact
# samples) the residual r = c - F13 - sign(F13) / 16, F13 = M X M^T / 8 the transform with the IJG constants in real arithmetic and the
# last term the mean of the quantiser's ties, is rounding noise of standard deviation below SIGMA_Q1; an encoder whose constant k is
# off by e units has r = e P_k + noise with P_k = (S_k X M^T + M X S_k^T) / 8, S_k the change of the pass per unit of k.  The least-squares
# e_k = <r, P_k> / <P_k, P_k> has standard deviation SIGMA_Q1 / |P_k|; with |P_k| >= 10 SIGMA_Q1 / 0.5 a constant one unit off lies ten
# standard deviations from zero and the limit 5 sigma lies half-way.
# SIGMA_Q1^2: the quantiser's residues k / 8, k = -3 ... 4, have mean square 44 / 512; the islow roundings add (1 / 12 + 1 / 24) / 64
# (pass 2's own, and pass 1's eight through sum_y M[v, y]^2 / 16 = 1 / 2) -- 0.0879, so 0.3 is above its root.
SIGMA_Q1 = 0.3


def swing_noise(nby: int, nbx: int, seed: int) -> np.ndarray:
    """a grey image of nby x nbx blocks at full swing: every pixel 0 or 240 at random, plus 0 ... 15 (the multiplicands of the
    constants are large, the rounding residues spread)"""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 2, (nby * 8, nbx * 8)) * 240 + rng.integers(0, 16, (nby * 8, nbx * 8))).astype(np.uint8)


def constant_estimates(coef_zz: np.ndarray, img: np.ndarray) -> dict:
    """{constant: (units the encoder's constant lies from the IJG one, 5 sigma of that estimate)} from the quality-100 coefficients
    of a grey image; over the coefficients with |F13| >= 1"""
    a = img if img.ndim == 3 else img[..., None]
    assert a.shape[2] == 1
    x = sample_blocks(a)[0] - 128.0
    _, m = islow_matrices()
    f13 = m @ x @ m.T / 8.0
    c = np.zeros((len(x), 64), np.float64)
    c[:, ZIGZAG] = coef_zz
    keep = np.abs(f13) >= 1.0
    r = np.where(keep, c.reshape(-1, 8, 8) - f13 - np.sign(f13) * TIE_BIAS, 0.0)
    out = {}
    for name in ISLOW_13BIT:
        k = dict(ISLOW_13BIT)
        k[name] += 2.0 ** -CONST_BITS
        s = _flow(np.eye(8), k) - m
        p = np.where(keep, (s @ x @ m.T + m @ x @ s.T) / 8.0, 0.0)
        pp = float((p * p).sum())
        out[name] = (float((r * p).sum()) / pp, 5.0 * SIGMA_Q1 / np.sqrt(pp))
    return out


# ----------------------------------------------------------------------------------------------------------------------- inputs
def cells(h: int, w: int, base: np.ndarray | None = None, seed: int = 0) -> np.ndarray:
    """An even-sized BGR image without a single ambiguous sample, built 2 x 2 cell by cell by rejection: a cell is kept only if none of
    its twelve conversions lies within EPS_C of a tie and neither chroma sum is 2 (mod 4).  ``base`` None: uniform noise; else the
    (h, w, 3) base perturbed by -3 ... 3 per value.  About two draws per cell."""
    assert h % 2 == 0 and w % 2 == 0
    rng = np.random.default_rng(seed)
    out = np.zeros((h // 2, w // 2, 2, 2, 3), np.uint8)
    todo = np.ones((h // 2, w // 2), bool)
    b = None if base is None else base.reshape(h // 2, 2, w // 2, 2, 3).transpose(0, 2, 1, 3, 4).astype(np.int64)
    for _ in range(200):
        n = int(todo.sum())
        if n == 0:
            break
        draw = rng.integers(0, 256, (n, 2, 2, 3)) if b is None else np.clip(b[todo] + rng.integers(-3, 4, (n, 2, 2, 3)), 0, 255)
        planes = ycc(draw.reshape(n, 4, 3).astype(np.float64))
        ok = np.ones(n, bool)
        for k, v in enumerate(planes):
            ok &= (np.abs(v - np.floor(v) - 0.5) > EPS_C).all(1) & (v < 255.5 - EPS_C).all(1)
            if k:
                ok &= np.rint(v).sum(1).astype(np.int64) % 4 != 2
        idx = np.argwhere(todo)[ok]
        out[idx[:, 0], idx[:, 1]] = draw[ok].astype(np.uint8)
        todo[idx[:, 0], idx[:, 1]] = False
    assert not todo.any()
    return np.ascontiguousarray(out.transpose(0, 2, 1, 3, 4).reshape(h, w, 3))
