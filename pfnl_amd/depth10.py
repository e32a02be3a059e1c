"""Frames at 10 bits, out and in: quantisation, resampling and YUV 4:2:0 / 4:2:2 / 4:4:4 both ways, stated once in integers (numpy and Python integers
only; no device).

The network's result is fp32; the streaming session can deliver it at 10 bits instead of 8 (include/pfnl_hip.h, pfnl_stream_format with
PFNL_PIX_RGB10 / PFNL_PIX_P010 / PFNL_PIX_I010; pfnl_amd/csrc/depth10.hip), and this module is the rule its kernels are tested against,
sample for sample.  Samples are little-endian uint16 and there is one depth, 10 bits.  The three steps are the 8-bit ones (pfnl_amd/model.py
quantise, pfnl_amd/resize.py, pfnl_amd/yuv.py) with the wider sample:

* ``quantise10``: round(clip(sr * 1023, 0, 1023)), the product in float32 as on the device (an fp64 product rounds about 15 per million
  uniform inputs to the neighbouring code), round half to even.  Inputs are finite or +-inf; for NaN the device delivers 0 (its fmax
  returns the other operand), numpy's clip would keep the NaN: that case is documented here and compared nowhere;
* ``resize10``: the tap tables of resize.taps unchanged - 14 fractional bits, rows that sum to 2^14, sum |c| <= 2^15 - and another split
  of the fixed point: h = (sum c p + 2^9) >> 10 (4 fractional bits, unclipped, |h| <= 1023 * 2^15 / 2^10 = 32736 fits int16), then
  clip((sum c h + 2^17) >> 18, 0, 1023) (|sum| <= 32736 * 2^15 < 2^31);
* ``from_rgb10``: the construction of yuv.coefficients with the 10-bit ranges - limited: 64 .. 940 luma (ys = 876 / 1023), 64 .. 960 chroma
  (cs = 896 / 1023); full: 0 .. 1023 - Y = clip((yr R + yg G + yb B + (y0 << 14) + 2^13) >> 14, 0, 1023); the chroma numerators stay
  unrounded until the 1-2-1 filter over columns 2i - 1, 2i, 2i + 1 (clamped) of both luma rows has summed them, then
  clip(512 + ((S + 2^16) >> 17), 0, 1023): chroma sited left, as yuv.downsample.  |S| + (512 << 17) + 2^16 < 2^31.  With another
  ``siting`` (yuv.SITINGS) the filter is yuv.encode_filter's and the rounding (S + 2^(13 + k)) >> (14 + k), k = 2 for "center" and 4 for
  "topleft": |S| <= 1023 * 2^14 * 16 stays below 2^31 with the offset and the rounding term.

Layouts (tightly packed, H * W * 3 / 2 samples, H and W even): ``p010`` = Y [H][W], CbCr [H/2][W/2][2], every sample value << 6 (the low six
bits zero); ``i010`` (yuv420p10le) = Y, Cb [H/2][W/2], Cr [H/2][W/2], every sample the value itself; ``rgb10`` = [H][W][3], values 0 .. 1023.

The input side (pfnl_stream_input_depth; pfnl_amd/csrc/yuv.hip decode, stream.hip 16-bit ring) has three more functions, lenient where
``planes10`` is strict - a decoder's surface is taken as it comes:

* ``values10``: the sample values as the device takes them - p010: sample >> 6, the low six bits ignored; i010 / rgb10: min(sample, 1023).
  The clamp is part of the rule: no kernel indexes a table or multiplies with an unclamped sample;
* ``to_rgb10``: yuv.to_rgb with ``decode_coefficients10`` (the same construction, ys = 876 / 1023, cs = 896 / 1023, y0 = 64), the chroma
  offset 512 and the clip at 1023; chroma at every luma pixel by yuv.upsample, whose arithmetic does not depend on the depth;
* ``dequantise10``: v / 1023 in double, rounded once to float32 - what the network sees of a 10-bit sample.

With ``chroma`` "422" / "444" (yuv.CHROMAS) the same two layouts hold chroma planes of [H][W/2] / [H][W] - ``p010`` is then P210 / P410,
``i010`` yuv422p10le / yuv444p10le; 2 H W / 3 H W samples - and the rule is yuv.py's: no filter along an axis that is not subsampled.

Out of scope: BT.2020 and transfer functions, 12 and 16 bits, monochrome, 4:1:1 and alpha, pitched planes, sitings other than yuv.SITINGS.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

from . import resize as _resize
from . import yuv as _yuv

BITS = 10
MAXV = (1 << BITS) - 1                                                  # 1023
F = _yuv.F
HALF = _yuv.HALF
FORMATS = ("p010", "i010")                                              # the 4:2:0 layouts ("rgb10" is the third 10-bit output)
MATRICES = {k: _yuv.MATRICES[k] for k in ("bt601", "bt709")}
SHIFT = {"p010": 16 - BITS, "i010": 0}                                  # where a value sits in its uint16


# ---- quantisation ------------------------------------------------------------------------------------------------------------------------
def quantise10(sr):
    """fp32 in any shape -> uint16 in [0, 1023]: the float32 product, clipped, rounded half to even."""
    sr = np.asarray(sr)
    return np.round(np.clip(sr.astype(np.float32) * np.float32(MAXV), 0, MAXV)).astype(np.uint16)


# ---- YUV 4:2:0 ---------------------------------------------------------------------------------------------------------------------------
def coefficients10(matrix: str, full_range) -> Tuple[int, Tuple[int, ...]]:
    """(y0, encode): encode = (yr, yg, yb, cbr, cbg, cbb, crr, crg, crb) - the ten integers of pfnl_yuv10_coefficients, in its order."""
    if matrix not in MATRICES:
        raise ValueError(f"matrix: one of {sorted(MATRICES)}, got {matrix!r}")
    kr, kb = MATRICES[matrix]
    if full_range:
        y0, ys, cs = 0, 1.0, 1.0
    else:
        y0, ys, cs = 64, 876.0 / 1023.0, 896.0 / 1023.0
    rnd = _yuv._rnd
    yr, yb = rnd(ys * kr), rnd(ys * kb)
    yg = rnd(ys) - yr - yb
    cbr, cbb = rnd(-cs * kr / (2.0 * (1.0 - kb))), rnd(cs / 2.0)
    cbg = -cbr - cbb
    crr, crb = rnd(cs / 2.0), rnd(-cs * kb / (2.0 * (1.0 - kr)))
    crg = -crr - crb
    return y0, (yr, yg, yb, cbr, cbg, cbb, crr, crg, crb)


def decode_coefficients10(matrix: str, full_range) -> Tuple[int, Tuple[int, ...]]:
    """(y0, decode): decode = (dy, drv, dgu, dgv, dbu) - the six integers of pfnl_yuv10_decode_coefficients, in its order."""
    if matrix not in MATRICES:
        raise ValueError(f"matrix: one of {sorted(MATRICES)}, got {matrix!r}")
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    if full_range:
        y0, ys, cs = 0, 1.0, 1.0
    else:
        y0, ys, cs = 64, 876.0 / 1023.0, 896.0 / 1023.0
    rnd = _yuv._rnd
    dy = rnd(1.0 / ys)
    drv, dbu = rnd(2.0 * (1.0 - kr) / cs), rnd(2.0 * (1.0 - kb) / cs)
    dgu, dgv = rnd(-2.0 * kb * (1.0 - kb) / (kg * cs)), rnd(-2.0 * kr * (1.0 - kr) / (kg * cs))
    return y0, (dy, drv, dgu, dgv, dbu)


def _geometry(fmt: str, H: int, W: int, chroma="420") -> None:
    if fmt not in FORMATS:
        raise ValueError(f"fmt: one of {FORMATS}, got {fmt!r}")
    _yuv.check_size(H, W, chroma)


def frame_samples(H: int, W: int, chroma="420") -> int:
    return _yuv.frame_bytes(H, W, chroma)


def planes10(frame, fmt: str, H: int, W: int, chroma="420"):
    """(Y [H,W], Cb [H/2,W/2], Cr [H/2,W/2]) uint16 VALUES in [0, 1023] of one packed frame (any shape with H*W*3/2 samples; Cb and Cr
    [H,W/2] of 2 H W samples at 4:2:2, [H,W] of 3 H W at 4:4:4).  ValueError
    for a sample that is no 10-bit value in its place: above 1023 (i010), or with one of the low six bits set (p010)."""
    _geometry(fmt, H, W, chroma)
    ch, cw = _yuv.chroma_shape(H, W, chroma)
    flat = np.asarray(frame).reshape(-1)
    if flat.dtype != np.uint16 or flat.size != frame_samples(H, W, chroma):
        raise ValueError(f"expected {frame_samples(H, W, chroma)} uint16 samples, got {flat.dtype} x {flat.size}")
    sh = SHIFT[fmt]
    if sh and (flat & ((1 << sh) - 1)).any():
        raise ValueError(f"{fmt}: the low {sh} bits of every sample are zero")
    flat = flat >> sh
    if flat.size and int(flat.max()) > MAXV:
        raise ValueError(f"{fmt}: values above {MAXV}")
    y = flat[:H * W].reshape(H, W)
    c = flat[H * W:]
    if fmt == "p010":
        c = c.reshape(ch, cw, 2)
        return y, c[..., 0], c[..., 1]
    c = c.reshape(2, ch, cw)
    return y, c[0], c[1]


def pack10(Y, Cb, Cr, fmt: str, chroma="420"):
    """[H*3/2, W] uint16 ([2H, W] at 4:2:2, [3H, W] at 4:4:4): the planes (values in [0, 1023]) as one packed frame."""
    Y, Cb, Cr = (np.asarray(p) for p in (Y, Cb, Cr))
    if Y.ndim != 2:
        raise ValueError("Y must be [H, W]")
    H, W = Y.shape
    _geometry(fmt, H, W, chroma)
    if Cb.shape != _yuv.chroma_shape(H, W, chroma) or Cr.shape != Cb.shape:
        raise ValueError("Cb and Cr must be [H/2, W/2]" if chroma == "420" else f"Cb and Cr must be {list(_yuv.chroma_shape(H, W, chroma))}")
    for p in (Y, Cb, Cr):
        if p.size and (int(p.min()) < 0 or int(p.max()) > MAXV):
            raise ValueError(f"values must lie in 0 .. {MAXV}")
    Y, Cb, Cr = (p.astype(np.uint16) for p in (Y, Cb, Cr))
    c = np.stack([Cb, Cr], axis=-1) if fmt == "p010" else np.stack([Cb, Cr], axis=0)
    return (np.concatenate([Y.reshape(-1), c.reshape(-1)]) << SHIFT[fmt]).astype(np.uint16).reshape(frame_samples(H, W, chroma) // W, W)


IN_FORMATS = FORMATS + ("rgb10",)                                       # what values10 takes


def values10(frame, fmt: str, chroma="420"):
    """The sample values of a packed 10-bit frame as the device takes them, uint16 in [0, 1023], in the frame's shape: ``p010`` sample >> 6
    (the low six bits are ignored), ``i010`` / ``rgb10`` min(sample, 1023).  Lenient where planes10 refuses.  The rule is per sample, so
    ``chroma`` (checked against yuv.CHROMAS) changes nothing: P210 / P410 are taken as P010 is."""
    _yuv.chroma_id(chroma)
    if fmt not in IN_FORMATS:
        raise ValueError(f"fmt: one of {IN_FORMATS}, got {fmt!r}")
    frame = np.asarray(frame)
    if frame.dtype != np.uint16:
        raise ValueError(f"expected uint16 samples, got {frame.dtype}")
    return frame >> SHIFT["p010"] if fmt == "p010" else np.minimum(frame, np.uint16(MAXV))


def to_rgb10(frame, fmt: str, H: int, W: int, matrix: str = "bt709", full_range=False, siting="left", chroma="420"):
    """One packed ``p010`` / ``i010`` frame (any shape with H*W*3/2 uint16 samples - 2 H W | 3 H W at 4:2:2 | 4:4:4 - taken by values10) ->
    [H,W,3] uint16 in [0, 1023]."""
    _geometry(fmt, H, W, chroma)
    y0, (dy, drv, dgu, dgv, dbu) = decode_coefficients10(matrix, full_range)
    flat = np.asarray(frame).reshape(-1)
    if flat.dtype != np.uint16 or flat.size != frame_samples(H, W, chroma):
        raise ValueError(f"expected {frame_samples(H, W, chroma)} uint16 samples, got {flat.dtype} x {flat.size}")
    Y, Cb, Cr = planes10(values10(flat, fmt) << SHIFT[fmt], fmt, H, W, chroma)
    yy = dy * (Y.astype(np.int64) - y0)
    u = _yuv.upsample(Cb, H, W, siting, chroma).astype(np.int64) - 512
    v = _yuv.upsample(Cr, H, W, siting, chroma).astype(np.int64) - 512
    nums = np.stack([yy + drv * v, yy + dgu * u + dgv * v, yy + dbu * u], axis=-1) + HALF
    assert np.abs(nums).max() < (1 << 31)                               # (over the whole sample cube: at most 36 085 868 + 2^13)
    return np.clip(nums >> F, 0, MAXV).astype(np.uint16)


def dequantise10(v):
    """uint16 in any shape -> float32 in [0, 1]: min(v, 1023) / 1023, the division in double and rounded once - the 10-bit twin of the
    harness's (u8 / 255.).astype(np.float32)."""
    v = np.asarray(v)
    if v.dtype != np.uint16:
        raise ValueError(f"expected uint16 samples, got {v.dtype}")
    return (np.minimum(v, np.uint16(MAXV)).astype(np.float64) / float(MAXV)).astype(np.float32)


def downsample10(N, siting="left", chroma="420"):
    """Chroma numerators [H,W] (14 fractional bits, unrounded) -> the plane [H/2, W/2] ([H, W/2] | [H, W]) of values: the siting's filter
    (left: 1-2-1 over two rows), one rounding."""
    s, k = _yuv.encode_filter(np.asarray(N, np.int64), siting, chroma)
    assert np.abs(s).max() + (512 << (F + k)) + (1 << (F + k - 1)) < (1 << 31)
    return np.clip(512 + ((s + (1 << (F + k - 1))) >> (F + k)), 0, MAXV).astype(np.uint16)


def _check_rgb10(rgb10):
    rgb10 = np.asarray(rgb10)
    if rgb10.dtype != np.uint16 or rgb10.ndim != 3 or rgb10.shape[2] != 3:
        raise ValueError(f"expected [H,W,3] uint16, got {rgb10.dtype} {rgb10.shape}")
    if rgb10.size and int(rgb10.max()) > MAXV:
        raise ValueError(f"values above {MAXV}")
    return rgb10


def from_rgb10(rgb10, fmt: str, matrix: str = "bt709", full_range=False, siting="left", chroma="420"):
    """[H,W,3] uint16 with values <= 1023 -> one packed frame [H*3/2, W] uint16 in ``fmt`` ([2H, W] at 4:2:2, [3H, W] at 4:4:4)."""
    rgb10 = _check_rgb10(rgb10)
    H, W = rgb10.shape[:2]
    _geometry(fmt, H, W, chroma)
    y0, (yr, yg, yb, cbr, cbg, cbb, crr, crg, crb) = coefficients10(matrix, full_range)
    r, g, b = (rgb10[..., k].astype(np.int64) for k in range(3))
    Y = np.clip((yr * r + yg * g + yb * b + (y0 << F) + HALF) >> F, 0, MAXV)
    Cb = downsample10(cbr * r + cbg * g + cbb * b, siting, chroma)
    Cr = downsample10(crr * r + crg * g + crb * b, siting, chroma)
    return pack10(Y, Cb, Cr, fmt, chroma)


# ---- resampling --------------------------------------------------------------------------------------------------------------------------
def resize10_passes(frame, out_h: int, out_w: int):
    """(h, v): the horizontal pass [H, out_w, 3] (4 fractional bits) and the second pass's SUM [out_h, out_w, 3] ahead of its rounding, int64"""
    frame = _check_rgb10(frame)
    H, W = frame.shape[:2]
    h = (_resize._apply(frame, _resize.taps(W, out_w), 1) + (1 << 9)) >> 10
    assert np.abs(h).max() < (1 << 15)
    return h, _resize._apply(h, _resize.taps(H, out_h), 0)


def resize10_unclipped(frame, out_h: int, out_w: int):
    """The second pass ahead of its clip, [out_h, out_w, 3] int64: values outside [0, 1023] are the overshoot the clip removes."""
    v = resize10_passes(frame, out_h, out_w)[1]
    assert np.abs(v).max() + (1 << 17) < (1 << 31)
    return (v + (1 << 17)) >> 18


def resize10(frame, out_h: int, out_w: int):
    """[H,W,3] uint16 with values <= 1023 -> [out_h, out_w, 3] uint16."""
    return np.clip(resize10_unclipped(frame, out_h, out_w), 0, MAXV).astype(np.uint16)


# ---- placement on a canvas (pfnl_amd/fit.py) -----------------------------------------------------------------------------------------------
def fill10(fill) -> Tuple[int, int, int]:
    """An 8-bit fill colour at 10 bits: (v << 2) | (v >> 6) per channel, so 0 -> 0 and 255 -> 1023 (bit replication)."""
    from . import fit as _fit
    return tuple((v << 2) | (v >> 6) for v in _fit.as_fill(fill))


def place10(frame, out_h: int, out_w: int, src=None, dst=None, fill=(0, 0, 0)):
    """fit.place on 10-bit samples: [H,W,3] uint16 with values <= 1023 -> [out_h, out_w, 3] uint16, ``fill10(fill)`` everywhere - ``fill``
    is the 8-bit colour - and resize10(frame[src], dst.h, dst.w) at ``dst``."""
    from . import fit as _fit
    return _fit._place(_check_rgb10(frame), out_h, out_w, src, dst, fill10(fill), np.uint16, resize10)
