"""Tiled forward: the rule, stated once, in numpy and Python integers (no device).

A large frame runs as a batch of overlapping tiles of one shape.  A tiling is ``(tile_h, tile_w, pad, batch)``; the device side
(pfnl_forward_tiled, pfnl_amd/csrc/tiles.hip, pfnl_amd/csrc/tile_geom.h) is tested against this module byte for byte.

Per axis of length n (even), tile extent t and margin p:

    t == 0 or t >= n    one tile [0, n) that owns all of it
    otherwise           t even, p >= 0, 2p < t;  step = t - 2p;  count = ceil((n - 2p) / step);
                        origin o_i = min(i * step, n - t)   (the last tile moves inward: every tile has extent t and an even origin)
                        tile i owns [a_i, b_i):  a_0 = 0,  a_i = o_i + p,  b_i = a_(i+1),  b_last = n

so the owned ranges partition [0, n) and every owned sample lies at least p from each tile edge that is not a frame edge.  The same pad
serves both axes.  The tiles of a call [B,T,H,W,3] are numbered clip-major, then by row of tiles, then by column: (b * ny + iy) * nx + ix.
They run in runs of ``batch`` consecutive tiles (the last run may be shorter; batch == 0: all tiles in one run), each run one forward at
[run,T,th,tw,3]; the output is the owned rectangle of each tile's result, scaled by ``scale``, at its place: every output element is
written exactly once, nothing is blended.

With pad >= 4 + 2 * num_block (the receptive field of the trunk and the tail, the halo pfnl_forward_strip recomputes) the tiled result
differs from the full-frame forward only through the non-local block, which sees its own tile instead of the frame.
"""
from __future__ import annotations

import numpy as np

INT_MAX = 2 ** 31 - 1


def _int(v, name) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"tile: {name} must be an integer, got {v!r}")
    return int(v)


def tiling(tile):
    """``(th, tw)``, ``(th, tw, pad)`` or ``(th, tw, pad, batch)`` as the 4-tuple of Python integers; ValueError for any other form or a
    negative entry.  (What fits a frame: ``check``.)"""
    if isinstance(tile, (str, bytes)) or not hasattr(tile, "__len__") or not 2 <= len(tile) <= 4:
        raise ValueError(f"tile must be (th, tw), (th, tw, pad) or (th, tw, pad, batch), got {tile!r}")
    t = [_int(v, n) for v, n in zip(tile, ("tile_h", "tile_w", "pad", "batch"))] + [0, 0][:4 - len(tile)]
    for v, n in zip(t, ("tile_h", "tile_w", "pad", "batch")):
        if v < 0 or v > INT_MAX:
            raise ValueError(f"tile: {n} must lie in 0 .. 2^31 - 1, got {v}")
    return tuple(t)


def count(n, t, p) -> int:
    """The number of tiles of one axis; ValueError for an (n, t, p) the rule does not cover."""
    n, t, p = _int(n, "n"), _int(t, "tile"), _int(p, "pad")
    if n <= 0 or n % 2:
        raise ValueError(f"tile: the axis length n must be positive and even, got {n}")
    if t < 0 or t % 2:
        raise ValueError(f"tile: the tile extent must be even and not negative, got {t}")
    if p < 0:
        raise ValueError(f"tile: pad must not be negative, got {p}")
    if t == 0 or t >= n:
        return 1
    if 2 * p >= t:
        raise ValueError(f"tile: 2 * pad must be smaller than the tile extent where the axis is split, got pad {p}, tile {t}")
    return -(-(n - 2 * p) // (t - 2 * p))


def axis(n, t, p):
    """The tiles of one axis as ``[(origin, own_first, own_end), ...]``; each has extent ``t``, or ``n`` where the axis is not split."""
    count_ = count(n, t, p)
    n, t, p = int(n), int(t), int(p)
    if count_ == 1:
        return [(0, 0, n)]
    step = t - 2 * p
    origin = [min(i * step, n - t) for i in range(count_)]
    first = [0] + [o + p for o in origin[1:]]
    return [(o, a, b) for o, a, b in zip(origin, first, first[1:] + [n])]


def grid(H, W, tile):
    """``(th, tw, rows, cols)``: the tile shape and the two axes (``axis``) of a frame of H x W."""
    th, tw, pad, _ = tiling(tile)
    rows, cols = axis(H, th, pad), axis(W, tw, pad)
    return (th if len(rows) > 1 else int(H)), (tw if len(cols) > 1 else int(W)), rows, cols


def check(H, W, tile):
    """The 4-tuple of a tiling that fits a frame of H x W; ValueError for what ``tiling_refused`` (tile_geom.h) refuses."""
    t = tiling(tile)
    if count(H, t[0], t[2]) * count(W, t[1], t[2]) > INT_MAX:
        raise ValueError("tile: the tile count overflows a 32-bit integer")
    return t


def runs(total, batch):
    """``[(first, count), ...]``: runs of ``batch`` consecutive tiles, a shorter last one; batch == 0: one run."""
    total, batch = _int(total, "total"), _int(batch, "batch")
    if total < 1 or batch < 0:
        raise ValueError(f"tile: total must be positive and batch not negative, got {total}, {batch}")
    step = total if batch == 0 else batch
    return [(f, min(step, total - f)) for f in range(0, total, step)]


def split(x, tile):
    """x [B,T,H,W,3] -> the tile stack [B * ny * nx, T, th, tw, 3], clip-major, then rows of tiles, then columns.  A contiguous copy."""
    x = np.asarray(x)
    if x.ndim != 5:
        raise ValueError(f"expected [B,T,H,W,3], got shape {x.shape}")
    B, T, H, W, C = x.shape
    check(H, W, tile)
    th, tw, rows, cols = grid(H, W, tile)
    out = np.empty((B * len(rows) * len(cols), T, th, tw, C), x.dtype)
    k = 0
    for b in range(B):
        for oy, _, _ in rows:
            for ox, _, _ in cols:
                out[k] = x[b, :, oy:oy + th, ox:ox + tw]
                k += 1
    return out


def assemble(ys, B, H, W, scale, tile):
    """The owned rectangle of every tile's result at its place.  ``ys``: the results of all tiles [B * ny * nx, ..., s*th, s*tw, C], or
    the list of the runs' results in order; returns [B, ..., s*H, s*W, C] (the axes between the first and the last three are kept)."""
    ys = np.concatenate([np.asarray(y) for y in ys]) if isinstance(ys, (list, tuple)) else np.asarray(ys)
    check(H, W, tile)
    th, tw, rows, cols = grid(H, W, tile)
    s = _int(scale, "scale")
    if s < 1 or ys.ndim < 4 or ys.shape[0] != B * len(rows) * len(cols) or ys.shape[-3:-1] != (s * th, s * tw):
        raise ValueError(f"expected {B * len(rows) * len(cols)} tile results of {s * th} x {s * tw}, got shape {ys.shape}")
    out = np.empty((B,) + ys.shape[1:-3] + (s * H, s * W, ys.shape[-1]), ys.dtype)
    k = 0
    for b in range(B):
        for oy, ay, by in rows:
            for ox, ax, bx in cols:
                out[b, ..., s * ay:s * by, s * ax:s * bx, :] = ys[k, ..., s * (ay - oy):s * (by - oy), s * (ax - ox):s * (bx - ox), :]
                k += 1
    return out


def forward_tiled(f, x, tile):
    """The tiled forward of any callable ``f`` ([n,T,th,tw,3] -> [n,...,s*th,s*tw,C], any n): run after run of ``split(x)`` through ``f``,
    assembled.  The scale is read off the first result."""
    x = np.asarray(x)
    t = check(x.shape[-3], x.shape[-2], tile)
    stack = split(x, t)
    ys = [np.asarray(f(np.ascontiguousarray(stack[a:a + n]))) for a, n in runs(len(stack), t[3])]
    return assemble(ys, x.shape[0], x.shape[-3], x.shape[-2], ys[0].shape[-3] // stack.shape[-3], t)
