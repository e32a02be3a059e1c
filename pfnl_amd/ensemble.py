"""Geometric self-ensemble: the rule, stated once, in numpy (no device).

The "+" row of a super-resolution table: the network runs on the 8 flips and transposes of its input, each result is transformed back
and the results are averaged.  The device side (pfnl_forward_ensemble, pfnl_amd/csrc/dihedral.hip) is tested against this module byte
for byte.

Members are k = 0 .. 7 and act on the axes H, W of an array [..., H, W, 3]: bit 0 mirrors W, bit 1 mirrors H, bit 2 transposes H and W
and is applied last.  ``inverse`` undoes the steps in reverse order.  An ensemble of n in {1, 2, 4, 8} uses members 0 .. n-1: 2 is the
horizontal mirror, 4 both mirrors (the geometry unchanged), 8 adds the transposes, which run the network at W x H.  The result is

    acc = f(x);  for k = 1 .. n-1: acc = fl32(acc + inverse(f(transform(x, k)), k));  out = acc * (1 / n)

with fp32 accumulation in increasing k and an exact scale (1 / n is a power of two).  n = 1 is f itself.
"""
from __future__ import annotations

import numpy as np

SIZES = (1, 2, 4, 8)


def members(n) -> range:
    """The members of an ensemble of ``n``: 0 .. n-1.  ValueError unless n is 1, 2, 4 or 8."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or int(n) not in SIZES:
        raise ValueError(f"ensemble must be 1, 2, 4 or 8, got {n!r}")
    return range(int(n))


def _member(k) -> int:
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= int(k) <= 7:
        raise ValueError(f"member k must lie in 0 .. 7, got {k!r}")
    return int(k)


def transform(x, k):
    """g_k(x) on the last three axes [..., H, W, 3]; [..., W, H, 3] for k >= 4.  A contiguous copy."""
    k = _member(k)
    a = np.asarray(x)
    if a.ndim < 3:
        raise ValueError(f"expected [..., H, W, 3], got shape {a.shape}")
    if k & 1:
        a = a[..., :, ::-1, :]
    if k & 2:
        a = a[..., ::-1, :, :]
    if k & 4:
        a = a.swapaxes(-3, -2)
    return np.ascontiguousarray(a)


def inverse(y, k):
    """g_k^-1(y): the transpose first, then the mirrors.  inverse(transform(x, k), k) == x."""
    k = _member(k)
    a = np.asarray(y)
    if a.ndim < 3:
        raise ValueError(f"expected [..., H, W, 3], got shape {a.shape}")
    if k & 4:
        a = a.swapaxes(-3, -2)
    if k & 2:
        a = a[..., ::-1, :, :]
    if k & 1:
        a = a[..., :, ::-1, :]
    return np.ascontiguousarray(a)


def combine(forward, x, n):
    """The ensemble of ``n`` members of any callable ``forward`` (array [..., H, W, 3] -> array [..., H', W', 3] that maps the H and W
    axes to the H' and W' axes), accumulated in float32 in increasing k and scaled by 1 / n.  n = 1 returns float32(forward(x))."""
    ks = members(n)
    acc = np.array(forward(np.asarray(x)), dtype=np.float32)
    for k in ks[1:]:
        acc = acc + inverse(np.asarray(forward(transform(x, k)), dtype=np.float32), k)   # float32 + float32: one rounding per member
    return acc * np.float32(1.0 / len(ks)) if len(ks) > 1 else acc
