"""YUV 4:2:0 / 4:2:2 / 4:4:4 <-> RGB, 8 bits, stated once in integers (numpy only; no device).

The streaming session takes and delivers NV12 / I420 frames (include/pfnl_hip.h, pfnl_stream_format; pfnl_amd/csrc/yuv.hip); this module is
the rule its kernels are tested against, byte for byte.  Everything after the coefficients is integer arithmetic:

* F = 14 fractional bits, ONE = 1 << 14, rnd(x) = floor(x * ONE + 0.5); every coefficient is computed in double precision and rounded once,
  the third of each encode row is derived from the other two - greys have zero chroma and white is y0 + round(255 ys) exactly;
* frames are tightly packed, H * W * 3 / 2 bytes, H and W even: ``nv12`` = Y [H][W], CbCr [H/2][W/2][2]; ``i420`` = Y, Cb [H/2][W/2], Cr;
* chroma is sited left by default (H.264 / HEVC type 0): on the even luma columns, midway between the two luma rows.  YUV -> RGB
  interpolates it with the weights 3 : 1 vertically (near row : far row) and 1 : 1 between two samples on odd columns, indices clamped to
  the plane; RGB -> YUV filters the unrounded chroma numerators with 1-2-1 over the two luma rows, columns clamped, and rounds once;
* ``siting`` names where chroma sample (j, i) sits in luma coordinates (row, column): "left" (2j + 1/2, 2i), "center" (2j + 1/2, 2i + 1/2;
  JPEG / MPEG-1, Y4M's C420jpeg), "topleft" (2j, 2i; HEVC type 2, C420paldv).  Per axis a siting is midway or co-sited (AXES).  Decode: two
  taps per axis in quarters, indices clamped - midway: near = j, far = j + 1 on odd and j - 1 on even luma indices, 3 : 1; co-sited: near =
  j, far = j + 1, 4 : 0 on even and 2 : 2 on odd indices - and (sum wy wx C + 8) >> 4.  Encode: per axis a box over 2j, 2j + 1 (midway, k =
  1) or 1-2-1 over 2j - 1, 2j, 2j + 1 (co-sited, k = 2), indices clamped, and one rounding by F + k bits, k summed over both axes;
* ``chroma`` names the subsampling (CHROMAS): "420" as above, "422" (chroma planes [H][W/2]: NV16 = Y [H][W], CbCr [H][W/2][2]; I422 = Y, Cb
  [H][W/2], Cr; 2 H W bytes, W even, any H) or "444" ([H][W]: NV24 = Y, CbCr [H][W][2]; I444 = three planes; 3 H W bytes, any H, W).  The rule
  is the one above per axis, and an axis that is not subsampled takes no filter at all: decode, the sample itself along it, so 4:2:2 is
  (w_near C[near] + w_far C[far] + 2) >> 2 and 4:4:4 is C; encode, k = 0 along it, so 4:4:4 is (N + HALF) >> F.  The siting is read for
  its horizontal axis alone at 4:2:2 ("left" and "topleft" are one rule there) and not at all at 4:4:4.

Out of scope: pitched planes (pfnl_amd/surface.py), 10 bits (input and output: pfnl_amd/depth10.py), monochrome, 4:1:1 and alpha, sitings other than these
three (HEVC types 1, 3, 4, 5), transfer functions, BT.2020.
"""
from __future__ import annotations

import math
from typing import Tuple

import numpy as np

F = 14
ONE = 1 << F
HALF = ONE >> 1
FORMATS = ("nv12", "i420")
SITINGS = ("left", "center", "topleft")                               # PFNL_SITING_*: the index is the C-ABI's value
AXES = {"left": (True, False), "center": (True, True), "topleft": (False, False)}   # (vertical, horizontal): midway? (else co-sited)
CHROMAS = ("420", "422", "444")                                       # PFNL_CHROMA_*: the index is the C-ABI's value
SUBSAMPLED = {"420": (True, True), "422": (False, True), "444": (False, False)}   # (vertical, horizontal): half as many chroma samples?
MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}       # Kr, Kb


def _rnd(x: float) -> int:
    return int(math.floor(x * ONE + 0.5))


def coefficients(matrix: str, full_range) -> Tuple[int, Tuple[int, ...], Tuple[int, ...]]:
    """(y0, encode, decode): encode = (yr, yg, yb, cbr, cbg, cbb, crr, crg, crb), decode = (dy, drv, dgu, dgv, dbu) - the fifteen
    integers of pfnl_yuv_coefficients, in its order."""
    if matrix not in MATRICES:
        raise ValueError(f"matrix: one of {sorted(MATRICES)}, got {matrix!r}")
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    if full_range:
        y0, ys, cs = 0, 1.0, 1.0
    else:
        y0, ys, cs = 16, 219.0 / 255.0, 224.0 / 255.0
    yr, yb = _rnd(ys * kr), _rnd(ys * kb)
    yg = _rnd(ys) - yr - yb
    cbr, cbb = _rnd(-cs * kr / (2.0 * (1.0 - kb))), _rnd(cs / 2.0)
    cbg = -cbr - cbb
    crr, crb = _rnd(cs / 2.0), _rnd(-cs * kb / (2.0 * (1.0 - kr)))
    crg = -crr - crb
    dy = _rnd(1.0 / ys)
    drv, dbu = _rnd(2.0 * (1.0 - kr) / cs), _rnd(2.0 * (1.0 - kb) / cs)
    dgu, dgv = _rnd(-2.0 * kb * (1.0 - kb) / (kg * cs)), _rnd(-2.0 * kr * (1.0 - kr) / (kg * cs))
    return y0, (yr, yg, yb, cbr, cbg, cbb, crr, crg, crb), (dy, drv, dgu, dgv, dbu)


def chroma_id(chroma) -> int:
    """The C-ABI's PFNL_CHROMA_* value of a subsampling's name; ValueError for anything else."""
    if chroma not in CHROMAS:
        raise ValueError(f"chroma: one of {CHROMAS}, got {chroma!r}")
    return CHROMAS.index(chroma)


def check_size(H: int, W: int, chroma="420") -> None:
    """ValueError unless a frame of H x W exists at this subsampling: a subsampled axis is even and at least 2, any other at least 1."""
    vsub, hsub = SUBSAMPLED[CHROMAS[chroma_id(chroma)]]
    if vsub and hsub:
        if H < 2 or W < 2 or H % 2 or W % 2:
            raise ValueError(f"H and W must be even and at least 2, got {H} x {W}")
    elif hsub:
        if H < 1 or W < 2 or W % 2:
            raise ValueError(f"4:2:2: W must be even and at least 2 and H at least 1, got {H} x {W}")
    elif H < 1 or W < 1:
        raise ValueError(f"4:4:4: H and W must be at least 1, got {H} x {W}")


def _geometry(fmt: str, H: int, W: int, chroma="420") -> None:
    if fmt not in FORMATS:
        raise ValueError(f"fmt: one of {FORMATS}, got {fmt!r}")
    check_size(H, W, chroma)


def chroma_shape(H: int, W: int, chroma="420") -> Tuple[int, int]:
    """The rows and columns of one chroma plane of an H x W frame."""
    vsub, hsub = SUBSAMPLED[CHROMAS[chroma_id(chroma)]]
    return (H // 2 if vsub else H, W // 2 if hsub else W)


def frame_bytes(H: int, W: int, chroma="420") -> int:
    ch, cw = chroma_shape(H, W, chroma)
    return H * W + 2 * ch * cw


def planes(frame, fmt: str, H: int, W: int, chroma="420"):
    """(Y [H,W], Cb, Cr) uint8 of one packed frame (any shape with frame_bytes elements); Cb and Cr are [H/2,W/2] at 4:2:0, [H,W/2] at
    4:2:2 and [H,W] at 4:4:4."""
    _geometry(fmt, H, W, chroma)
    flat = np.asarray(frame).reshape(-1)
    if flat.dtype != np.uint8 or flat.size != frame_bytes(H, W, chroma):
        raise ValueError(f"expected {frame_bytes(H, W, chroma)} uint8 elements, got {flat.dtype} x {flat.size}")
    ch, cw = chroma_shape(H, W, chroma)
    y = flat[:H * W].reshape(H, W)
    c = flat[H * W:]
    if fmt == "nv12":
        c = c.reshape(ch, cw, 2)
        return y, c[..., 0], c[..., 1]
    c = c.reshape(2, ch, cw)
    return y, c[0], c[1]


def pack(Y, Cb, Cr, fmt: str, chroma="420"):
    """[H*3/2, W] uint8 ([2H, W] at 4:2:2, [3H, W] at 4:4:4): the planes as one packed frame."""
    Y, Cb, Cr = (np.asarray(p, np.uint8) for p in (Y, Cb, Cr))
    H, W = Y.shape
    _geometry(fmt, H, W, chroma)
    if Cb.shape != chroma_shape(H, W, chroma) or Cr.shape != Cb.shape:
        raise ValueError("Cb and Cr must be [H/2, W/2]" if chroma == "420" else f"Cb and Cr must be {list(chroma_shape(H, W, chroma))}")
    c = np.stack([Cb, Cr], axis=-1) if fmt == "nv12" else np.stack([Cb, Cr], axis=0)
    return np.concatenate([Y.reshape(-1), c.reshape(-1)]).reshape(frame_bytes(H, W, chroma) // W, W)


def siting_id(siting) -> int:
    """The C-ABI's PFNL_SITING_* value of a siting's name; ValueError for anything else."""
    if siting not in SITINGS:
        raise ValueError(f"siting: one of {SITINGS}, got {siting!r}")
    return SITINGS.index(siting)


def _decode_taps(n: int, midway: bool):
    """(near, far, w_near, w_far) per luma index 0 .. n - 1 of one axis: chroma indices clamped to n / 2, weights in quarters."""
    y = np.arange(n)
    j = y >> 1
    if midway:
        far, wn, wf = np.where(y & 1, j + 1, j - 1), np.full(n, 3), np.full(n, 1)
    else:
        far, wn, wf = j + 1, np.where(y & 1, 2, 4), np.where(y & 1, 2, 0)
    return j, np.clip(far, 0, n // 2 - 1), wn, wf


def upsample(C, H: int, W: int, siting="left", chroma="420"):
    """One chroma plane [H/2, W/2] at every luma pixel, [H,W] int32 in the plane's range ([0, 255]; the arithmetic does not depend on the
    depth: depth10.to_rgb10 calls it with values up to 1023).  ``chroma``: the plane is [H, W/2] ("422": the horizontal taps alone, in
    quarters) or [H, W] ("444": the plane itself)."""
    vmid, hmid = AXES[SITINGS[siting_id(siting)]]
    vsub, hsub = SUBSAMPLED[CHROMAS[chroma_id(chroma)]]
    C = np.asarray(C).astype(np.int32)
    if C.shape != chroma_shape(H, W, chroma):
        raise ValueError(f"expected a plane of {chroma_shape(H, W, chroma)}, got {C.shape}")
    bits = 0                                                            # two per filtered axis: the weights are quarters
    if vsub:
        jn, jf, wyn, wyf = _decode_taps(H, vmid)
        C, bits = wyn[:, None] * C[jn] + wyf[:, None] * C[jf], bits + 2  # [H, W/2]
    if hsub:
        i_n, i_f, wxn, wxf = _decode_taps(W, hmid)
        C, bits = wxn[None, :] * C[:, i_n] + wxf[None, :] * C[:, i_f], bits + 2
    return (C + (1 << (bits - 1))) >> bits if bits else C


def to_rgb(frame, fmt: str, H: int, W: int, matrix: str = "bt709", full_range=False, siting="left", chroma="420"):
    """One packed frame -> [H,W,3] uint8."""
    y0, _, (dy, drv, dgu, dgv, dbu) = coefficients(matrix, full_range)
    Y, Cb, Cr = planes(frame, fmt, H, W, chroma)
    yy = dy * (Y.astype(np.int32) - y0)
    u, v = upsample(Cb, H, W, siting, chroma) - 128, upsample(Cr, H, W, siting, chroma) - 128
    r = (yy + drv * v + HALF) >> F
    g = (yy + dgu * u + dgv * v + HALF) >> F
    b = (yy + dbu * u + HALF) >> F
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


def encode_filter(N, siting="left", chroma="420"):
    """(s, k): the chroma numerators [H,W] filtered per axis onto [H/2, W/2] - a box over 2j, 2j + 1 on a midway axis, 1-2-1 over 2j - 1, 2j,
    2j + 1 (clamped) on a co-sited one - unrounded, in N's integer type, and the bits k its weights add: the sum of the weights is 1 << k.
    An axis that ``chroma`` does not subsample is left as it is and adds no bits: [H, W/2] at "422", N itself and k = 0 at "444"."""
    vmid, hmid = AXES[SITINGS[siting_id(siting)]]
    vsub, hsub = SUBSAMPLED[CHROMAS[chroma_id(chroma)]]
    N = np.asarray(N)
    k = 0
    for axis, mid, sub in ((0, vmid, vsub), (1, hmid, hsub)):
        if not sub:
            continue
        n = N.shape[axis]
        c = np.arange(0, n, 2)
        if mid:
            N = np.take(N, c, axis) + np.take(N, c + 1, axis)
        else:
            N = np.take(N, np.clip(c - 1, 0, n - 1), axis) + 2 * np.take(N, c, axis) + np.take(N, c + 1, axis)
        k += 1 if mid else 2
    return N, k


def downsample(N, siting="left", chroma="420"):
    """Chroma numerators [H,W] int32 (14 fractional bits, unrounded) -> the plane [H/2, W/2] uint8 ([H, W/2] | [H, W]): the siting's
    filter (left: 1-2-1 over two rows), one rounding."""
    s, k = encode_filter(np.asarray(N, np.int32), siting, chroma)
    return np.clip(128 + ((s + (1 << (F + k - 1))) >> (F + k)), 0, 255).astype(np.uint8)


def from_rgb(rgb, fmt: str, matrix: str = "bt709", full_range=False, siting="left", chroma="420"):
    """[H,W,3] uint8 -> one packed frame [H*3/2, W] uint8 ([2H, W] at 4:2:2, [3H, W] at 4:4:4)."""
    rgb = np.asarray(rgb)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError(f"expected [H,W,3] uint8, got {rgb.dtype} {rgb.shape}")
    H, W = rgb.shape[:2]
    _geometry(fmt, H, W, chroma)
    y0, (yr, yg, yb, cbr, cbg, cbb, crr, crg, crb), _ = coefficients(matrix, full_range)
    r, g, b = (rgb[..., k].astype(np.int32) for k in range(3))
    Y = np.clip((yr * r + yg * g + yb * b + (y0 << F) + HALF) >> F, 0, 255)
    Cb = downsample(cbr * r + cbg * g + cbb * b, siting, chroma)
    Cr = downsample(crr * r + crg * g + crb * b, siting, chroma)
    return pack(Y, Cb, Cr, fmt, chroma)
