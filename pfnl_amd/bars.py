"""Letterbox and pillarbox bars, stated once on the host (numpy and Python integers only, no device): where the picture of a frame is.

The device kernel (pfnl_amd/csrc/bars.hip; include/pfnl_hip.h BARS) runs this rule on ring frames and the tests compare it with these
functions; the integer steps behind the sums (threshold, scan, union, snap, decide) are written once more in pfnl_amd/csrc/bars_geom.h.

A frame's luma is scene.luma_u8 / scene.luma_u10: integer BT.601 on the 8-bit scale without its + 16, so black is 0 and white 219 | 220.
A row is *picture* iff the sum of its luma exceeds ``limit * W``, a column iff its sum exceeds ``limit * H`` - a mean above ``limit``,
compared as sums so that no quotient is ever rounded.  The box runs from the first to the last picture row and column.  The default
limit 8 is ffmpeg cropdetect's 24 on a Y that starts at 16.
"""
from __future__ import annotations

from typing import Iterable, Sequence, Tuple

import numpy as np

from . import scene

LIMIT = 8                      # the default limit
LIMIT_MAX = 219                # the luma of white at 8 bits: a row can be no brighter
MAX_SIDE = 16384               # 220 * 16384 < 2^32: the device's sums are 32-bit
MIN_KEEP = (1, 3)              # decide(): the least fraction of either axis a crop may keep

Box = Tuple[int, int, int, int]
EMPTY: Box = (0, 0, 0, 0)


def check_limit(limit) -> int:
    if isinstance(limit, bool) or not isinstance(limit, (int, np.integer)) or not 0 <= int(limit) <= LIMIT_MAX:
        raise ValueError(f"limit: an integer in 0 .. {LIMIT_MAX}, got {limit!r}")
    return int(limit)


def line_sums(frame, depth: int = 8):
    """[H,W,3] RGB (uint8, or uint16 at 10 bits) -> (rows [H], cols [W]) int64: the sums of luma along each row and each column."""
    if depth not in (8, 10):
        raise ValueError(f"depth: 8 or 10, got {depth!r}")
    y = (scene.luma_u10 if depth == 10 else scene.luma_u8)(frame)
    if y.shape[0] > MAX_SIDE or y.shape[1] > MAX_SIDE:
        raise ValueError(f"H and W are at most {MAX_SIDE}")
    return y.sum(axis=1, dtype=np.int64), y.sum(axis=0, dtype=np.int64)


def _span(sums, n: int, thr: int):
    at = [i for i in range(n) if int(sums[i]) > thr]
    return (at[0], at[-1]) if at else None


def box(rows, cols, H: int, W: int, limit: int = LIMIT) -> Box:
    """(y0, x0, h, w): first to last picture row and column; (0, 0, 0, 0) with no picture row or no picture column."""
    limit = check_limit(limit)
    H, W = int(H), int(W)
    if len(rows) != H or len(cols) != W:
        raise ValueError("rows has H entries and cols W")
    r, c = _span(rows, H, limit * W), _span(cols, W, limit * H)
    if r is None or c is None:
        return EMPTY
    return (r[0], c[0], r[1] - r[0] + 1, c[1] - c[0] + 1)


def frame_box(frame, limit: int = LIMIT, depth: int = 8) -> Box:
    rows, cols = line_sums(frame, depth)
    return box(rows, cols, len(rows), len(cols), limit)


def _is_empty(b) -> bool:
    return int(b[2]) <= 0 or int(b[3]) <= 0


def union(boxes: Iterable[Sequence[int]]) -> Box:
    """The bounding box of the non-empty boxes; all empty (or none): (0, 0, 0, 0)."""
    got = [tuple(int(v) for v in b) for b in boxes]
    got = [b for b in got if not _is_empty(b)]
    if not got:
        return EMPTY
    y0, x0 = min(b[0] for b in got), min(b[1] for b in got)
    y1, x1 = max(b[0] + b[2] for b in got), max(b[1] + b[3] for b in got)
    return (y0, x0, y1 - y0, x1 - x0)


def snap(b: Sequence[int], ay: int, ax: int) -> Box:
    """The box shrunk inward onto multiples of ay rows and ax columns: start rounded up, end rounded down; a box that vanishes is empty."""
    ay, ax = int(ay), int(ax)
    if ay < 1 or ax < 1:
        raise ValueError("snap: the grid is at least 1 x 1")
    if _is_empty(b):
        return EMPTY
    y0, x0, h, w = (int(v) for v in b)
    y1, x1 = (y0 + h) // ay * ay, (x0 + w) // ax * ax
    y0, x0 = -(-y0 // ay) * ay, -(-x0 // ax) * ax
    if y1 <= y0 or x1 <= x0:
        return EMPTY
    return (y0, x0, y1 - y0, x1 - x0)


def align(chroma, interlaced: bool = False) -> Tuple[int, int]:
    """(ay, ax), the grid a crop ahead of the network lies on: the network needs even H and W, a field its parity kept and whole chroma
    rows.  chroma: "420" for 4:2:0 planes, anything else (None, "422", "444": RGB and planes with full-height chroma) otherwise;
    interlaced: the frames are woven (interlaced= or telecine=)."""
    return (4 if (str(chroma) == "420" and interlaced) else 2, 2)


def decide(boxes: Iterable[Sequence[int]], H: int, W: int, ay: int, ax: int, min_keep: Tuple[int, int] = MIN_KEEP) -> Box:
    """The crop a probe yields: snap(union(boxes)), or the whole frame (0, 0, H, W) where that is empty or keeps less than
    min_keep = (p, q) - the fraction p / q, a policy and no measurement - of either axis: a probe that saw only a fade-in must not crop
    the film away."""
    H, W = int(H), int(W)
    p, q = (int(v) for v in min_keep)
    if q < 1 or not 0 <= p <= q:
        raise ValueError("min_keep: a fraction (p, q) with 0 <= p <= q")
    y0, x0, h, w = snap(union(boxes), ay, ax)
    if h <= 0 or w <= 0 or y0 + h > H or x0 + w > W or h * q < H * p or w * q < W * p:
        return (0, 0, H, W)
    return (y0, x0, h, w)


def parse_crop(text: str):
    """--crop: "auto", or "Y,X,H,W" -> a box of input pixels."""
    if text == "auto":
        return "auto"
    parts = text.split(",")
    try:
        vals = tuple(int(p) for p in parts)
    except ValueError:
        vals = ()
    if len(vals) != 4:
        raise ValueError(f"crop: auto or Y,X,H,W in input pixels, got {text!r}")
    return vals


def check_crop(b: Sequence[int], H: int, W: int, ay: int, ax: int) -> Box:
    """A crop named by the user: inside the frame, not empty, on align()'s grid - else ValueError naming the reason."""
    y0, x0, h, w = (int(v) for v in b)
    if h < 1 or w < 1 or y0 < 0 or x0 < 0 or y0 + h > H or x0 + w > W:
        raise ValueError(f"crop {y0},{x0},{h},{w} lies outside the {H} x {W} frame")
    if y0 % ay or h % ay or x0 % ax or w % ax:
        raise ValueError(f"crop {y0},{x0},{h},{w} is off the grid: rows in multiples of {ay}, columns in multiples of {ax}")
    return (y0, x0, h, w)
