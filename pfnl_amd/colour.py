"""The colour of the streaming session's two edges, stated once on the host: primaries, the gamut matrix between two sets of them, the
transfer tables, and the per-pixel rule the device follows sample for sample (pfnl_amd/csrc/colour_geom.h, colour.hip; include/pfnl_hip.h
COLOUR).  numpy, Python integers and ``fractions``; nothing here needs a device.

A DVD's picture is SMPTE-C (NTSC) or EBU (PAL) primaries under a BT.601 matrix; an HD stream is read as BT.709 in both.  Matrix and range
are arguments of the YUV conversions (pfnl_amd/yuv.py); the primaries need linear light:

    ``out = E[clip((M . D[rgb] + 2^13) >> 14, 0, 65535)]``

per pixel - D the sample -> 16-bit linear light table, M ``gamut_matrix(src, dst)`` with 14 fractional bits, E the linear -> sample table.
All three systems share the BT.709 transfer curve and the white point D65, so there is no chromatic adaptation, ``E[D[v]] == v`` and every
row of M sums to 2^14: greys pass untouched.
"""
from __future__ import annotations

import functools
import math
from fractions import Fraction
from typing import List, Tuple

import numpy as np

PRIMARIES = ("bt709", "bt601-525", "bt601-625")                       # the index is the C-ABI value, PFNL_PRIM_*
XY = {                                                                # CIE 1931 x, y of R, G, B
    "bt709": ((Fraction(640, 1000), Fraction(330, 1000)), (Fraction(300, 1000), Fraction(600, 1000)), (Fraction(150, 1000), Fraction(60, 1000))),
    "bt601-525": ((Fraction(630, 1000), Fraction(340, 1000)), (Fraction(310, 1000), Fraction(595, 1000)), (Fraction(155, 1000), Fraction(70, 1000))),   # SMPTE 170M
    "bt601-625": ((Fraction(640, 1000), Fraction(330, 1000)), (Fraction(290, 1000), Fraction(600, 1000)), (Fraction(150, 1000), Fraction(60, 1000))),   # BT.470BG
}
WHITE = (Fraction(3127, 10000), Fraction(3290, 10000))                # D65, for all three
FRAC = 14                                                             # fractional bits of the matrix
ONE = 1 << FRAC
LINEAR_TOP = 65535                                                    # linear light is 16 bits
ALPHA, BETA = 1.09929682680944, 0.018053968510807                     # the BT.709 OETF: 4.5 L below BETA, else ALPHA L^0.45 - (ALPHA - 1)
BUCKET = 6                                                            # the device's form of E: the code at the start of each 2^BUCKET-wide bucket of l ...
BUCKETS = (LINEAR_TOP + 1) >> BUCKET                                  # ... 1024 of them, and the thresholds (encode_form)


def primaries_id(name) -> int:
    """The C-ABI value of a name of PRIMARIES; ValueError for anything else."""
    if not isinstance(name, str) or name not in PRIMARIES:
        raise ValueError(f"primaries: one of {PRIMARIES}, got {name!r}")
    return PRIMARIES.index(name)


def _inverse(m):
    """The inverse of a 3 x 3 matrix of Fractions, by the adjugate."""
    (a, b, c), (d, e, f), (g, h, i) = m
    det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)
    adj = [[e * i - f * h, c * h - b * i, b * f - c * e],
           [f * g - d * i, a * i - c * g, c * d - a * f],
           [d * h - e * g, b * g - a * h, a * e - b * d]]
    return [[v / det for v in row] for row in adj]


def _mul(a, b):
    return [[sum(a[r][k] * b[k][c] for k in range(3)) for c in range(3)] for r in range(3)]


def rgb_to_xyz(name: str) -> List[List[Fraction]]:
    """RGB -> XYZ of a set of primaries with white D65 mapped from (1, 1, 1), in exact rationals."""
    primaries_id(name)
    cols = [(x / y, Fraction(1), (1 - x - y) / y) for x, y in XY[name]]
    p = [[cols[c][r] for c in range(3)] for r in range(3)]
    xw, yw = WHITE
    w = (xw / yw, Fraction(1), (1 - xw - yw) / yw)
    s = [sum(row[k] * w[k] for k in range(3)) for row in _inverse(p)]
    return [[p[r][c] * s[c] for c in range(3)] for r in range(3)]


def _round_away(q: Fraction) -> int:
    n = (abs(q.numerator) * 2 + q.denominator) // (2 * q.denominator)
    return n if q >= 0 else -n


@functools.lru_cache(maxsize=None)
def gamut_matrix(src: str, dst: str) -> Tuple[Tuple[int, int, int], ...]:
    """Linear RGB of ``src`` -> linear RGB of ``dst`` with 14 fractional bits: RGB -> XYZ of src, XYZ -> RGB of dst, in exact rationals;
    each entry times 2^14 rounded half away from zero; then each row's diagonal entry takes the residual, so the row sums to exactly 2^14.
    ``src == dst`` gives 2^14 I."""
    primaries_id(src), primaries_id(dst)
    m = _mul(_inverse(rgb_to_xyz(dst)), rgb_to_xyz(src))
    q = [[_round_away(v * ONE) for v in row] for row in m]
    for r in range(3):
        q[r][r] = ONE - sum(q[r][c] for c in range(3) if c != r)
    return tuple(tuple(row) for row in q)


def oetf(L: float) -> float:
    """The BT.709 OETF, linear light 0 .. 1 -> signal 0 .. 1."""
    return 4.5 * L if L < BETA else ALPHA * math.pow(L, 0.45) - (ALPHA - 1.0)


def oetf_inverse(V: float) -> float:
    """Its inverse, signal 0 .. 1 -> linear light 0 .. 1."""
    return V / 4.5 if V < 4.5 * BETA else math.pow((V + (ALPHA - 1.0)) / ALPHA, 1.0 / 0.45)


def _top(bits: int) -> int:
    if isinstance(bits, bool) or bits not in (8, 10):
        raise ValueError(f"bits: 8 or 10, got {bits!r}")
    return (1 << bits) - 1


@functools.lru_cache(maxsize=None)
def tables(bits: int = 8) -> Tuple[np.ndarray, np.ndarray]:
    """(D, E), both uint16 and read-only: ``D[v] = floor(65535 f^-1(v / top) + 0.5)`` for v = 0 .. top and ``E[l] = floor(top f(l / 65535) +
    0.5)`` for l = 0 .. 65535, f the BT.709 OETF, top = 255 or 1023; double arithmetic, ``math.pow``."""
    top = _top(bits)
    D = np.array([int(math.floor(LINEAR_TOP * oetf_inverse(v / top) + 0.5)) for v in range(top + 1)], np.uint16)
    E = np.array([int(math.floor(top * oetf(l / LINEAR_TOP) + 0.5)) for l in range(LINEAR_TOP + 1)], np.uint16)
    D.setflags(write=False)
    E.setflags(write=False)
    return D, E


@functools.lru_cache(maxsize=None)
def encode_form(bits: int = 8) -> Tuple[np.ndarray, np.ndarray, int]:
    """E as the device holds it, (start, threshold, steps): ``start[k] = E[64 k]`` for the 1024 buckets of l, ``threshold[c]`` the smallest l
    with ``E[l] >= c`` (threshold[0] = 0; E is monotone and takes every code), and the largest number of code boundaries inside one bucket -
    the bound of the compare loop of ``encode_lookup``."""
    top = _top(bits)
    E = tables(bits)[1].astype(np.int64)
    start = E[::1 << BUCKET].astype(np.uint16)
    threshold = np.searchsorted(E, np.arange(top + 1), side="left").astype(np.uint16)
    steps = int((E[(1 << BUCKET) - 1::1 << BUCKET] - E[::1 << BUCKET]).max())
    return start, threshold, steps


def encode_lookup(l, bits: int = 8) -> np.ndarray:
    """``E[l]`` the device's way: from the bucket's code, at most ``steps`` compares against the next code's threshold."""
    top = _top(bits)
    start, threshold, steps = encode_form(bits)
    l = np.asarray(l, np.int64)
    c = start[l >> BUCKET].astype(np.int64)
    thr = np.append(threshold.astype(np.int64), LINEAR_TOP + 1)         # (no code above top)
    for _ in range(steps):
        c = c + ((c < top) & (l >= thr[c + 1]))
    return c.astype(np.uint16)


def convert(rgb, src: str, dst: str, bits: int = 8) -> np.ndarray:
    """[..., 3] samples of ``bits`` bits in the primaries ``src`` -> the same picture in ``dst``: per pixel ``l = clip((M . D[rgb] + 2^13)
    >> 14, 0, 65535)`` per channel, the shift a floor, then ``E[l]``.  ``src == dst`` returns its input untouched."""
    top = _top(bits)
    primaries_id(src), primaries_id(dst)
    rgb = np.asarray(rgb)
    if rgb.shape[-1:] != (3,) or rgb.dtype != (np.uint8 if bits == 8 else np.uint16):
        raise ValueError(f"convert: [..., 3] {'uint8' if bits == 8 else 'uint16'} samples, got {rgb.dtype} {rgb.shape}")
    if src == dst:
        return rgb
    D, E = tables(bits)
    lin = D[np.minimum(rgb, top)].astype(np.int64)
    M = np.array(gamut_matrix(src, dst), np.int64)
    l = np.clip((lin @ M.T + (1 << (FRAC - 1))) >> FRAC, 0, LINEAR_TOP)
    return E[l].astype(rgb.dtype)


def convert_reference(rgb, src: str, dst: str, bits: int = 8) -> np.ndarray:
    """The same chain in double arithmetic with nothing rounded: [..., 3] samples -> [..., 3] float64 on the sample scale, clipped to
    0 .. top.  What ``convert`` is measured against."""
    top = _top(bits)
    m = np.array([[float(v) for v in row] for row in _mul(_inverse(rgb_to_xyz(dst)), rgb_to_xyz(src))])
    v = np.asarray(rgb, np.float64) / top
    lin = np.where(v < 4.5 * BETA, v / 4.5, np.power((v + (ALPHA - 1.0)) / ALPHA, 1.0 / 0.45))
    L = np.clip(lin @ m.T, 0.0, 1.0)
    return top * np.where(L < BETA, 4.5 * L, ALPHA * np.power(L, 0.45) - (ALPHA - 1.0))


def auto_primaries(height: int) -> str:
    """What a stream without a colour tag is taken to be: 480 / 486 lines bt601-525, 576 lines bt601-625, anything else bt709."""
    return "bt601-525" if height in (480, 486) else ("bt601-625" if height == 576 else "bt709")


def side_keywords(height: int, out_height: int, matrix: str, out_matrix=None, out_range=None, primaries=None, out_primaries=None) -> dict:
    """``open_stream``'s colour keywords for a command line's flags (pfnl_amd/upscale.py, pfnl_amd/rawvideo.py), each only where the caller
    names it (None: no such key, so a caller who names none opens the session it always opened).  ``primaries`` "auto": ``auto_primaries``
    of the input's height.  ``out_matrix`` / ``out_primaries`` "auto" go by the delivered height: above 576 lines "bt709", else the input's.
    ``out_range`` "limited" | "full" becomes ``out_full_range``.  ValueError for any other name."""
    kw = {}
    if primaries is not None:
        kw["primaries"] = auto_primaries(int(height)) if primaries == "auto" else PRIMARIES[primaries_id(primaries)]
    if out_matrix is not None:
        if out_matrix not in ("auto", "bt601", "bt709"):
            raise ValueError(f'out_matrix: "auto", "bt601" or "bt709", got {out_matrix!r}')
        kw["out_matrix"] = ("bt709" if int(out_height) > 576 else matrix) if out_matrix == "auto" else out_matrix
    if out_range is not None:
        if out_range not in ("limited", "full"):
            raise ValueError(f'out_range: "limited" or "full", got {out_range!r}')
        kw["out_full_range"] = out_range == "full"
    if out_primaries is not None:
        own = kw.get("primaries", "bt709")
        kw["out_primaries"] = ("bt709" if int(out_height) > 576 else own) if out_primaries == "auto" else PRIMARIES[primaries_id(out_primaries)]
    return kw
