"""Scenes of a streamed video, stated once on the host (numpy only, no device): where a scene begins and which frames a window may name.

The streaming session (include/pfnl_hip.h pfnl_stream_scenes; pfnl_amd/csrc/stream.hip) runs this rule on the device ring; the tests
compare it with these functions.  Each scene is a sequence of its own: its windows clamp at its first and last frame as the reference's
clamp at frame 0 and at the last frame of a clip on disk (model/pfnl.py:238-242) - with one scene the two rules are the same.

The detector is the usual mean absolute frame difference on integer BT.601 luma, compared as sums so that no quotient is ever rounded:
frame f >= 1 starts a scene when ``min(sad[f], |sad[f] - sad[f-1]|) >= ceil(threshold * H * W)``.  The second term keeps sustained fast
motion or flicker from firing on every frame, and the frame behind a cut (whose sad is back to normal, far below the cut's) from firing.
"""
from __future__ import annotations

import math
from typing import Iterable, Optional

import numpy as np


def luma_u8(frame) -> np.ndarray:
    """[H,W,3] uint8 RGB -> [H,W] int32: (66 R + 129 G + 25 B + 128) >> 8, integer BT.601 without its + 16 (only differences are used)."""
    f = np.asarray(frame)
    if f.dtype != np.uint8 or f.ndim != 3 or f.shape[2] != 3:
        raise ValueError(f"expected a [H,W,3] uint8 frame, got {f.dtype} {f.shape}")
    f = f.astype(np.int32)
    return (66 * f[..., 0] + 129 * f[..., 1] + 25 * f[..., 2] + 128) >> 8


def frame_sad(a, b) -> int:
    """sum |luma_u8(a) - luma_u8(b)| as a Python int: exact."""
    return int(np.abs(luma_u8(a) - luma_u8(b)).sum(dtype=np.int64))


def cut_rule(sad: int, sad_prev: int, thr_sum: int) -> bool:
    return min(int(sad), abs(int(sad) - int(sad_prev))) >= int(thr_sum)


def threshold_sum(threshold: float, H: int, W: int) -> int:
    """ceil(threshold * H * W): the sum a frame's sad is compared with; threshold = a mean luma difference in (0, 255]."""
    if not 0.0 < float(threshold) <= 255.0:
        raise ValueError("threshold must be in (0, 255]")
    return int(math.ceil(float(threshold) * int(H) * int(W)))


def frame_sads(frames_u8) -> list:
    """sad[f] of every frame against the one before it, cut or not; sad[0] = 0."""
    return [0] + [frame_sad(frames_u8[f], frames_u8[f - 1]) for f in range(1, len(frames_u8))]


def luma_u10(frame) -> np.ndarray:
    """[H,W,3] uint16 RGB at 10 bits (a sample above 1023 counts as 1023, depth10.values10) -> [H,W] int32:
    (66 R + 129 G + 25 B + 512) >> 10 - luma on the 8-BIT scale, one rounding, so that thresholds and sums mean what they mean at 8 bits."""
    f = np.asarray(frame)
    if f.dtype != np.uint16 or f.ndim != 3 or f.shape[2] != 3:
        raise ValueError(f"expected a [H,W,3] uint16 frame, got {f.dtype} {f.shape}")
    f = np.minimum(f, np.uint16(1023)).astype(np.int32)
    return (66 * f[..., 0] + 129 * f[..., 1] + 25 * f[..., 2] + 512) >> 10


def frame_sad10(a, b) -> int:
    """sum |luma_u10(a) - luma_u10(b)| as a Python int: exact."""
    return int(np.abs(luma_u10(a) - luma_u10(b)).sum(dtype=np.int64))


def frame_sads10(frames_u10) -> list:
    """frame_sads of 10-bit frames."""
    return [0] + [frame_sad10(frames_u10[f], frames_u10[f - 1]) for f in range(1, len(frames_u10))]


def scene_first(frames_u8, threshold: Optional[float] = None, marks: Iterable[int] = (), depth: int = 8) -> np.ndarray:
    """int64 [F]: the index of the first frame of each frame's scene.  Frame 0 starts scene 0 and is never a cut; frame f >= 1 starts a
    scene if it is in ``marks`` or, with a threshold, if cut_rule(sad[f], sad[f-1], threshold_sum) holds.  ``depth`` = 10: the frames are
    uint16 at 10 bits and the sums are frame_sads10's."""
    if depth not in (8, 10):
        raise ValueError(f"depth: 8 or 10, got {depth!r}")
    F = len(frames_u8)
    marks = set(int(m) for m in marks)
    out = np.zeros((F,), np.int64)
    if F == 0:
        return out
    sad = (frame_sads10 if depth == 10 else frame_sads)(frames_u8) if threshold is not None else [0] * F
    thr = threshold_sum(threshold, frames_u8[0].shape[0], frames_u8[0].shape[1]) if threshold is not None else 0
    for f in range(1, F):
        cut = f in marks or (threshold is not None and cut_rule(sad[f], sad[f - 1], thr))
        out[f] = f if cut else out[f - 1]
    return out


def scene_windows_index(scene_first, T: int, last: Optional[int] = None) -> np.ndarray:
    """[last + 1, T] int64 (last = F - 1 by default): window c, slot t = clamp(c + t - T//2, a, b) with a = scene_first[c] and b = the last
    frame of c's scene among the frames 0..last.  One scene: the index array of model.sliding_windows."""
    sf = np.asarray(scene_first, np.int64)
    last = len(sf) - 1 if last is None else int(last)
    if not -1 <= last < len(sf):
        raise ValueError("last must name a frame of the sequence")
    sf = sf[:last + 1]
    idx = np.zeros((last + 1, T), np.int64)
    for c in range(last + 1):
        b = c
        while b + 1 <= last and sf[b + 1] == sf[c]:
            b += 1
        idx[c] = np.clip(np.arange(c - T // 2, c - T // 2 + T), sf[c], b)
    return idx
