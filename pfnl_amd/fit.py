"""A source rectangle of a frame on a canvas: crop, letterbox and aspect fit, stated once in integers (numpy and Python integers only; no
device).

The streaming session can resample a rectangle of the network's raster into a rectangle of a canvas of chosen size and fill the rest with
one colour (include/pfnl_hip.h, pfnl_stream_place; pfnl_amd/csrc/place.hip); this module is the rule its kernel is tested against, byte
for byte, and the rule that turns "contain" / "cover" and a sample aspect ratio into the two rectangles.

* ``place(frame, out_h, out_w, src, dst, fill)``: the canvas filled with ``fill``, with ``resize.resize(frame[src], dst.h, dst.w)`` written
  at ``dst``.  It IS that composition: the taps clamp at the edges of the source rectangle, not of the frame, and no pixel outside ``src``
  reaches the output.  A rectangle is ``(y, x, h, w)``; None is the whole frame / the whole canvas.
* per axis the limits are resize.check_limits between the rectangles' sizes, ceil(n_in / 4) <= n_out <= 2 n_in; frame and canvas are at
  most 16384 a side; a rectangle has h, w >= 1 and lies inside its raster (``check_rects``: pfnl_amd/csrc/stream_route.h place_refused).
* ``rects(sH, sW, oH, oW, crop, fit, sar, g)`` -> (src, dst), with round(p / q) = (2 p + q) // (2 q), (cy, cx, ch, cw) = ``crop`` or the
  whole raster, A = cw sar[0], B = ch sar[1] (the picture is A : B on a display of square pixels), g = 2 for a 4:2:0 output, else 1 - or the grid per
  axis as (gy, gx): (1, 2) for a 4:2:2 output, (1, 1) for 4:4:4 and RGB; below, g is the grid of the axis it stands with:

  - fit None: src = crop, dst the whole canvas - the stretch of pfnl_stream_resize;
  - "contain", A oH >= B oW: w = oW, h = min(oH, g max(1, round(oW B / (g A)))); else h = oH, w = min(oW, g max(1, round(oH A / (g B))));
    y = ((oH - h) // (2 g)) g and x likewise; src = crop: the whole picture, bars on two sides, sizes and offsets multiples of g;
  - "cover": dst the whole canvas; A oH >= B oW: cw' = clamp(round(ch sar[1] oW / (oH sar[0])), 1, cw), cx += (cw - cw') // 2; else
    ch' = clamp(round(cw sar[0] oH / (oW sar[1])), 1, ch), cy += (ch - ch') // 2: the canvas is full, the picture loses two edges.

  A pair that breaks the per-axis limits raises ValueError.  The C-ABI takes rectangles only: this rule lives here.

The 10-bit form is pfnl_amd/depth10.py place10; a 4:2:0 output converts the canvas as it converts any frame (yuv.from_rgb), so black bars
leave as Y 16, chroma 128 by the existing rule.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

from . import resize as _resize

Rect = Tuple[int, int, int, int]


def as_rect(r, name: str, h: int, w: int) -> Rect:
    """``r`` as four Python integers, None as the whole h x w raster; ValueError for anything else."""
    if r is None:
        return 0, 0, int(h), int(w)
    try:
        y, x, rh, rw = (int(v) for v in r)
    except (TypeError, ValueError):
        raise ValueError(f"{name}: None or (y, x, h, w), got {r!r}") from None
    return y, x, rh, rw


def as_fill(fill, limit: int = 255) -> Tuple[int, int, int]:
    try:
        r, g, b = (int(v) for v in fill)
    except (TypeError, ValueError):
        raise ValueError(f"fill: (r, g, b), got {fill!r}") from None
    if not all(0 <= v <= limit for v in (r, g, b)):
        raise ValueError(f"fill: values in 0 .. {limit}, got {fill!r}")
    return r, g, b


def check_rects(sH: int, sW: int, oH: int, oW: int, src: Rect, dst: Rect) -> None:
    """ValueError where the library would refuse the pair (place_refused); the message names ``src`` or ``dst``."""
    for n in (sH, sW, oH, oW):
        if not 1 <= n <= _resize.MAX_SIZE:
            raise ValueError(f"place: raster and canvas sizes must lie in 1 .. {_resize.MAX_SIZE}, got {sH} x {sW} and {oH} x {oW}")
    for name, (y, x, h, w), (H, W) in (("src", src, (sH, sW)), ("dst", dst, (oH, oW))):
        if h < 1 or w < 1 or y < 0 or x < 0 or y + h > H or x + w > W:
            raise ValueError(f"place: {name} ({y}, {x}, {h}, {w}) must have h, w >= 1 and lie inside {H} x {W}")
    for n_in, n_out in ((src[2], dst[2]), (src[3], dst[3])):
        if not ((n_in + 3) // 4 <= n_out <= 2 * n_in):
            raise ValueError(f"place: src -> dst, {n_in} -> {n_out}: the output must lie between a quarter and twice the input")


def _place(frame, out_h: int, out_w: int, src, dst, fill, dtype, resize_fn):
    frame = np.asarray(frame)
    if frame.dtype != dtype or frame.ndim != 3 or frame.shape[2] != 3:
        raise ValueError(f"expected [H,W,3] {np.dtype(dtype).name}, got {frame.dtype} {frame.shape}")
    H, W = frame.shape[:2]
    out_h, out_w = int(out_h), int(out_w)
    src, dst = as_rect(src, "src", H, W), as_rect(dst, "dst", out_h, out_w)
    check_rects(H, W, out_h, out_w, src, dst)
    canvas = np.empty((out_h, out_w, 3), dtype)
    canvas[:] = np.asarray(fill, dtype)
    (sy, sx, sh, sw), (dy, dx, dh, dw) = src, dst
    canvas[dy:dy + dh, dx:dx + dw] = resize_fn(np.ascontiguousarray(frame[sy:sy + sh, sx:sx + sw]), dh, dw)
    return canvas


def place(frame, out_h: int, out_w: int, src: Optional[Rect] = None, dst: Optional[Rect] = None, fill=(0, 0, 0)):
    """[H,W,3] uint8 -> [out_h, out_w, 3] uint8: ``fill`` everywhere, resize.resize(frame[src], dst.h, dst.w) at ``dst``."""
    return _place(frame, out_h, out_w, src, dst, as_fill(fill), np.uint8, _resize.resize)


def _round_div(p: int, q: int) -> int:
    return (2 * p + q) // (2 * q)


def rects(sH: int, sW: int, oH: int, oW: int, crop: Optional[Rect] = None, fit: Optional[str] = None, sar=(1, 1), g: int = 1) -> Tuple[Rect, Rect]:
    """(src, dst) of a picture ``crop`` (None: the whole sH x sW raster) with sample aspect ratio ``sar`` on a canvas of oH x oW; see the
    module's text.  ValueError for an unknown ``fit``, a crop outside the raster and a pair outside the resampler's limits."""
    sH, sW, oH, oW = int(sH), int(sW), int(oH), int(oW)
    if fit not in (None, "contain", "cover"):
        raise ValueError(f'fit: None, "contain" or "cover", got {fit!r}')
    try:
        gy, gx = (int(v) for v in g) if isinstance(g, (tuple, list)) else (int(g), int(g))
    except (TypeError, ValueError):
        raise ValueError(f"g: 1, or 2 for a 4:2:0 output, or (gy, gx), got {g!r}") from None
    if gy not in (1, 2) or gx not in (1, 2):
        raise ValueError(f"g: 1, or 2 for a 4:2:0 output, got {g!r}")
    try:
        s0, s1 = (int(v) for v in sar)
    except (TypeError, ValueError):
        raise ValueError(f"sar: (num, den), got {sar!r}") from None
    if s0 < 1 or s1 < 1:
        raise ValueError(f"sar: two positive integers, got {sar!r}")
    cy, cx, ch, cw = as_rect(crop, "crop", sH, sW)
    if ch < 1 or cw < 1 or cy < 0 or cx < 0 or cy + ch > sH or cx + cw > sW:
        raise ValueError(f"place: src ({cy}, {cx}, {ch}, {cw}) must have h, w >= 1 and lie inside {sH} x {sW}")
    if oH < 1 or oW < 1:
        raise ValueError(f"place: the canvas must be at least 1 x 1, got {oH} x {oW}")
    A, B = cw * s0, ch * s1
    dst = (0, 0, oH, oW)
    if fit == "contain":
        if A * oH >= B * oW:
            w, h = oW, min(oH, gy * max(1, _round_div(oW * B, gy * A)))
        else:
            h, w = oH, min(oW, gx * max(1, _round_div(oH * A, gx * B)))
        dst = (((oH - h) // (2 * gy)) * gy, ((oW - w) // (2 * gx)) * gx, h, w)
    elif fit == "cover":
        if A * oH >= B * oW:
            cw2 = min(max(_round_div(ch * s1 * oW, oH * s0), 1), cw)
            cx, cw = cx + (cw - cw2) // 2, cw2
        else:
            ch2 = min(max(_round_div(cw * s0 * oH, oW * s1), 1), ch)
            cy, ch = cy + (ch - ch2) // 2, ch2
    src = (cy, cx, ch, cw)
    check_rects(sH, sW, oH, oW, src, dst)
    return src, dst
