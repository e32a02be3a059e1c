"""Resampling of uint8 RGB frames to a chosen raster, stated once in integers (numpy and Python integers only; no device).

The streaming session can deliver its SR frames at any size near the network's own (include/pfnl_hip.h, pfnl_stream_resize;
pfnl_amd/csrc/resize.hip); this module is the rule its kernel and its tap tables are tested against, byte for byte.  The filter is the
separable Keys cubic (a = -1/2) whose support widens by in / out when the raster shrinks - what Pillow's BICUBIC resize applies - with
every quantity an exact integer:

* one axis, ``taps(n_in, n_out)``: D = max(n_in, n_out), d = 2 D.  For output index o and any integer j, n = n_out (2 j + 1) -
  n_in (2 o + 1), u = |n|: the distance of sample j from the centre of o is u / d filter units.  The taps of o are the j with u < 2 d, and

      W = 3 u^3 - 5 u^2 d + 2 d^3            for u <= d
      W = -u^3 + 5 u^2 d - 8 u d^2 + 4 d^3   for d < u < 2 d

  (the Keys kernel times 2 d^3).  Indices are clamped to [0, n_in - 1] and the weights of taps that land on one sample are added: what
  remains is the run first[o] .. first[o] + count[o] - 1, and first and first + count never decrease with o;
* with S = sum W > 0: c_j = floor((2 W_j 2^14 + S) / (2 S)) - 14 fractional bits, half up, floor division for the negative ones as
  well - and the residue 2^14 - sum c goes to the largest c (the lowest j among equals): every row sums to 2^14 exactly;
* every row must hold sum |c| <= 2^15, which keeps the intermediate of a frame inside int16 and the second pass inside int32: a pair
  (n_in, n_out) that breaks it is refused;
* a frame, horizontal pass first: h = (sum_k ch[o][k] p[first + k] + 2^7) >> 8 per channel, arithmetic shift, 6 fractional bits and NOT
  clipped (overshoot survives into the second pass); then out = clip((sum_k cv[o][k] h[first + k] + 2^19) >> 20, 0, 255).

At the borders this rule clamps - as the bicubic skip and the chroma filters of this project do - where Pillow drops the taps outside the
frame and renormalises; in the interior the two differ by at most one level.  The library builds the same tables with 128-bit integers
(pfnl_resize_taps) for 1 <= n_in, n_out <= 16384 and ceil(n_in / 4) <= n_out <= 2 n_in; this module states the rule for any pair.

Cropping, letterboxing and aspect handling build on this rule in pfnl_amd/fit.py.  Out of scope: other filters, resampling ahead of the
quantisation.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

F = 14
ONE = 1 << F
MAX_ABS_SUM = 1 << 15
MAX_SIZE = 16384                                                        # the library's limits (pfnl_resize_taps)


def check_limits(n_in: int, n_out: int) -> None:
    """ValueError where the library would refuse the axis."""
    if not (1 <= n_in <= MAX_SIZE and 1 <= n_out <= MAX_SIZE):
        raise ValueError(f"sizes must lie in 1 .. {MAX_SIZE}, got {n_in} -> {n_out}")
    if not ((n_in + 3) // 4 <= n_out <= 2 * n_in):
        raise ValueError(f"{n_in} -> {n_out}: the output must lie between a quarter and twice the input")


def _weight(u: int, d: int) -> int:
    if u <= d:
        return 3 * u ** 3 - 5 * u * u * d + 2 * d ** 3
    if u < 2 * d:
        return -u ** 3 + 5 * u * u * d - 8 * u * d * d + 4 * d ** 3
    return 0


def _row(n_in: int, n_out: int, o: int):
    """(first, [c ...]) of output index o"""
    d = 2 * max(n_in, n_out)
    centre = n_in * (2 * o + 1)
    j = (centre - 2 * d - n_out) // (2 * n_out)                         # n_out (2 j + 1) <= centre - 2 d: the last one outside
    first, w = None, []
    while True:
        j += 1
        n = n_out * (2 * j + 1) - centre
        if n >= 2 * d:
            break
        if n <= -2 * d:
            continue
        at = min(max(j, 0), n_in - 1)
        if first is None:
            first = at
        if at - first == len(w):
            w.append(0)
        w[at - first] += _weight(abs(n), d)
    s = sum(w)
    assert first is not None and s > 0
    c = [(2 * x * ONE + s) // (2 * s) for x in w]
    c[c.index(max(c))] += ONE - sum(c)
    return first, c


def taps(n_in: int, n_out: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(first [n_out] int32, count [n_out] int32, coef [n_out, max_taps] int32, zero behind count): output o = sum_k coef[o, k] *
    in[first[o] + k] / 2^14.  ValueError where a row's sum of magnitudes exceeds 2^15."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f"sizes must be positive, got {n_in} -> {n_out}")
    rows = [_row(n_in, n_out, o) for o in range(n_out)]
    width = max(len(c) for _, c in rows)
    first = np.array([f for f, _ in rows], np.int32)
    count = np.array([len(c) for _, c in rows], np.int32)
    coef = np.zeros((n_out, width), np.int32)
    for o, (_, c) in enumerate(rows):
        if sum(abs(x) for x in c) > MAX_ABS_SUM:
            raise ValueError(f"{n_in} -> {n_out}: row {o} has sum |c| = {sum(abs(x) for x in c)} > {MAX_ABS_SUM}")
        coef[o, :len(c)] = c
    return first, count, coef


def max_taps(n_in: int, n_out: int) -> int:
    """The longest run of ``taps(n_in, n_out)`` (pfnl_resize_max_taps)."""
    return int(taps(n_in, n_out)[1].max())


def _apply(x, table, axis: int):
    """sum_k coef[o, k] * x[first[o] + k] along `axis`, int64"""
    first, count, coef = table
    x = np.moveaxis(np.asarray(x, np.int64), axis, 0)
    out = np.zeros((len(first),) + x.shape[1:], np.int64)
    tail = (1,) * (x.ndim - 1)
    for k in range(coef.shape[1]):
        idx = np.minimum(first + k, first + count - 1)                  # (behind count the coefficient is zero)
        out += coef[:, k].astype(np.int64).reshape((-1,) + tail) * x[idx]
    return np.moveaxis(out, 0, axis)


def resize_unclipped(frame, out_h: int, out_w: int):
    """The second pass ahead of its clip, [out_h, out_w, 3] int64: values outside [0, 255] are the overshoot the clip removes."""
    frame = np.asarray(frame)
    if frame.dtype != np.uint8 or frame.ndim != 3 or frame.shape[2] != 3:
        raise ValueError(f"expected [H,W,3] uint8, got {frame.dtype} {frame.shape}")
    H, W = frame.shape[:2]
    h = (_apply(frame, taps(W, out_w), 1) + (1 << 7)) >> 8
    assert np.abs(h).max() < (1 << 15)
    return (_apply(h, taps(H, out_h), 0) + (1 << 19)) >> 20


def resize(frame, out_h: int, out_w: int):
    """[H,W,3] uint8 -> [out_h, out_w, 3] uint8."""
    return np.clip(resize_unclipped(frame, out_h, out_w), 0, 255).astype(np.uint8)
