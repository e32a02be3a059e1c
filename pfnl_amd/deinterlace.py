"""Interlaced video in: the motion-adaptive deinterlacer ahead of the streaming session's ring, stated once on the host (include/pfnl_hip.h
INTERLACED; the kernel: csrc/deinterlace.hip; the index rules the session shares: csrc/field_geom.h).  numpy and Python integers only.

FIELDS.  A frame of H rows (H even) is two fields of h = H / 2 rows: the top field, parity 0, holds frame rows 0, 2, 4, ...; the bottom
field, parity 1, rows 1, 3, 5, ...  A sequence of N frames is 2 N fields in time order, k = 0 .. 2 N - 1: with ``field_order`` "tff" field
2 n is frame n's top field and field 2 n + 1 its bottom field, "bff" is the other way round.  A field index q outside [0, 2 N - 1] is
replaced by q + 2 (q < 0) or q - 2 (q > 2 N - 1): a field of the same parity, which always exists as 2 N >= 2.

THE PROGRESSIVE FRAME AT THE TIME OF FIELD k.  Field k has parity p and samples A; P1, N1 are fields k - 1, k + 1 (parity 1 - p: the rows
field k lacks), P2, N2 fields k - 2, k + 2 (parity p), after the replacement above.  Every sample is an integer in 0 .. MAX (255 | 1023; at
10 bits every sample read is min(v, 1023) first, depth10.values10); each of the 3 W samples of a row is handled alone - the rule has no
horizontal term.  Frame row 2 i + p is A[i].  Frame row 2 j + (1 - p), j = 0 .. h - 1, is the missing row: with u = j - p and every field
row index clamped to [0, h - 1],

    c = A[u], e = A[u + 1], cc = A[u - 1], ee = A[u + 2]
    s = clip((9 (c + e) - (cc + ee) + 8) >> 4, 0, MAX)            (floor; the numerator can be negative)
    x = P1[j], y = N1[j], d = (x + y + 1) >> 1
    t0 = |x - y|
    t1 = (|P2[u] - c| + |P2[u + 1] - e| + 1) >> 1
    t2 = (|N2[u] - c| + |N2[u + 1] - e| + 1) >> 1
    diff = max((t0 + 1) >> 1, t1, t2)
    out = min(max(s, d - diff), d + diff)

Where nothing moves diff = 0 and out = x: an exact weave.  Where the picture moves, out is the vertical cubic of the field's own rows, held
within diff of the temporal mean.  Every intermediate fits a signed 16-bit integer at both depths (|9 (c + e) + 8| <= 18 422).

RATES.  "frame": one output per input frame, at the time of its first field (k = 2 n); "field": one per field, 2 N frames.

DECODING.  A field is a picture of h rows: rows p, p + 2, ... of every plane of the pushed frame (Y, Cb, Cr, CbCr, the one plane of a
packing, an RGB plane), decoded by the functions the project already pins, called with H / 2.  For 4:2:2, 4:4:4, RGB and every packing that
equals decoding the woven frame; 4:2:0 alone filters vertically, and there a field's chroma rows belong to that field: H is a multiple of 4.
A field's 4:2:0 chroma is sited like a progressive picture's - the quarter-row offset of interlaced 4:2:0 siting is out of scope.
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np

from . import depth10 as _d10, packed as _packed, yuv as _yuv

FIELD_ORDERS = ("tff", "bff")                                           # PFNL_FIELD_*: the index is the C-ABI's value
RATES = ("frame", "field")                                              # PFNL_INTERLACE_FRAME, _FIELD are index + 1 (0: off)
BRANCHES = ("below", "inside", "above", "max_t0", "max_t1", "max_t2", "clip_low", "clip_high")


def order_id(field_order) -> int:
    if field_order not in FIELD_ORDERS:
        raise ValueError(f"field_order: one of {FIELD_ORDERS}, got {field_order!r}")
    return FIELD_ORDERS.index(field_order)


def mode_id(rate) -> int:
    """The C-ABI's PFNL_INTERLACE_* value of ``rate``: None 0 (off), "frame" 1, "field" 2; ValueError for anything else."""
    if rate is None:
        return 0
    if not isinstance(rate, str) or rate not in RATES:
        raise ValueError(f"interlaced: None or one of {RATES}, got {rate!r}")
    return RATES.index(rate) + 1


def check_height(H: int, chroma_420: bool = False) -> None:
    """ValueError unless a frame of H rows has two fields: H even and at least 2; with 4:2:0 planes a multiple of 4."""
    if H < 2 or H % 2:
        raise ValueError(f"interlaced: H must be even and at least 2, got {H}")
    if chroma_420 and H % 4:
        raise ValueError(f"interlaced: a 4:2:0 frame's fields need H to be a multiple of 4, got {H}")


def fields(plane) -> Tuple[np.ndarray, np.ndarray]:
    """(top, bottom): rows 0, 2, ... and rows 1, 3, ... of an array whose first axis is an even number of rows."""
    plane = np.asarray(plane)
    if plane.ndim < 1 or plane.shape[0] < 2 or plane.shape[0] % 2:
        raise ValueError("a frame has an even number of rows, at least 2")
    return plane[0::2], plane[1::2]


def field_sequence(n_frames: int, field_order="tff") -> List[Tuple[int, int]]:
    """(frame, parity) of the fields k = 0 .. 2 N - 1 in time order."""
    first = order_id(field_order)
    if n_frames < 1:
        raise ValueError("a sequence has at least one frame")
    return [(k >> 1, (k & 1) ^ first) for k in range(2 * n_frames)]


def replace(q: int, n_fields: int) -> int:
    """The field that stands for index q of a sequence of ``n_fields`` (even, >= 2) fields."""
    if n_fields < 2 or n_fields % 2 or q < -2 or q > n_fields + 1:
        raise ValueError("field index out of reach: -2 <= q <= n_fields + 1 of an even n_fields >= 2")
    return q + 2 if q < 0 else (q - 2 if q > n_fields - 1 else q)


def neighbours(k: int, n_fields: int) -> Tuple[int, int, int, int]:
    """(P2, P1, N1, N2): the fields k - 2, k - 1, k + 1, k + 2 after the replacement at the sequence's ends."""
    if not 0 <= k < n_fields:
        raise ValueError(f"field {k} of {n_fields}")
    return tuple(replace(k + o, n_fields) for o in (-2, -1, 1, 2))


def _terms(p2, p1, cur, n1, n2, parity: int, maxv: int) -> Dict[str, np.ndarray]:
    if parity not in (0, 1):
        raise ValueError(f"parity: 0 or 1, got {parity!r}")
    if maxv not in (255, 1023):
        raise ValueError(f"maxv: 255 or 1023, got {maxv!r}")
    f = [np.minimum(np.asarray(a).astype(np.int32), maxv) for a in (p2, p1, cur, n1, n2)]
    if f[2].ndim < 1 or f[2].shape[0] < 1 or any(a.shape != f[2].shape for a in f):
        raise ValueError("the five fields have one shape, [H / 2, ...]")
    if min(int(a.min()) for a in f) < 0:
        raise ValueError("samples are not negative")
    P2, P1, A, N1, N2 = f
    h = A.shape[0]
    u = np.arange(h) - parity
    at = lambda a, i: a[np.clip(i, 0, h - 1)]                           # noqa: E731
    c, e, cc, ee = at(A, u), at(A, u + 1), at(A, u - 1), at(A, u + 2)
    num = 9 * (c + e) - (cc + ee) + 8
    s = np.clip(num >> 4, 0, maxv)
    x, y = P1, N1
    d = (x + y + 1) >> 1
    t0 = (np.abs(x - y) + 1) >> 1
    t1 = (np.abs(at(P2, u) - c) + np.abs(at(P2, u + 1) - e) + 1) >> 1
    t2 = (np.abs(at(N2, u) - c) + np.abs(at(N2, u + 1) - e) + 1) >> 1
    diff = np.maximum(t0, np.maximum(t1, t2))
    return {"A": A, "num": num, "s": s, "d": d, "t0": t0, "t1": t1, "t2": t2, "diff": diff,
            "out": np.minimum(np.maximum(s, d - diff), d + diff)}


def interpolate(p2, p1, cur, n1, n2, parity: int, maxv: int = 255):
    """The progressive frame [H, ...] at the time of field ``cur`` [H / 2, ...] of parity ``parity``: uint8 for maxv 255, uint16 for 1023."""
    t = _terms(p2, p1, cur, n1, n2, parity, maxv)
    A = t["A"]
    out = np.empty((2 * A.shape[0],) + A.shape[1:], np.uint8 if maxv == 255 else np.uint16)
    out[parity::2] = A
    out[1 - parity::2] = t["out"]
    return out


def branches(p2, p1, cur, n1, n2, parity: int, maxv: int = 255) -> Dict[str, int]:
    """How many missing samples fall into each case of the rule (BRANCHES): s below / inside / above [d - diff, d + diff]; each of
    (t0 + 1) >> 1, t1, t2 the strict maximum; the cubic clipped at 0 and at MAX."""
    t = _terms(p2, p1, cur, n1, n2, parity, maxv)
    s, d, diff, a, b, c = t["s"], t["d"], t["diff"], t["t0"], t["t1"], t["t2"]
    return {"below": int((s < d - diff).sum()), "inside": int(((s >= d - diff) & (s <= d + diff)).sum()), "above": int((s > d + diff).sum()),
            "max_t0": int(((a > b) & (a > c)).sum()), "max_t1": int(((b > a) & (b > c)).sum()), "max_t2": int(((c > a) & (c > b)).sum()),
            "clip_low": int((t["num"] < 0).sum()), "clip_high": int(((t["num"] >> 4) > maxv).sum())}


def sequence_fields(rgb_frames: Sequence, field_order="tff") -> List[Tuple[np.ndarray, int]]:
    """(samples [H / 2, ...], parity) of the 2 N fields of N woven frames, in time order."""
    frames_ = [np.asarray(f) for f in rgb_frames]
    return [(fields(frames_[n])[p], p) for n, p in field_sequence(len(frames_), field_order)]


def frames(rgb_frames: Sequence, field_order="tff", rate="frame", maxv: int = 255) -> List[np.ndarray]:
    """The progressive frames of N woven frames [H, W, 3]: N of them at ``rate`` "frame", 2 N at "field"."""
    if rate not in RATES:
        raise ValueError(f"rate: one of {RATES}, got {rate!r}")
    seq = sequence_fields(rgb_frames, field_order)
    out = []
    for k in range(0, len(seq), 2 if rate == "frame" else 1):
        a, b, c, d = neighbours(k, len(seq))
        out.append(interpolate(seq[a][0], seq[b][0], seq[k][0], seq[c][0], seq[d][0], seq[k][1], maxv))
    return out


def field_frames(frame, pixel_format: str, H: int, W: int, in_depth: int = 8, chroma="420", packing=None) -> Tuple[np.ndarray, np.ndarray]:
    """(top, bottom): the two fields of a pushed frame as frames of H / 2 rows in the same layout - rows p, p + 2, ... of every plane."""
    if packing not in (None, "none"):
        check_height(H)
        rows = np.asarray(frame).reshape(-1).view(np.uint8).reshape(_packed.frame_shape(packing, H, W))
        return rows[0::2], rows[1::2]
    if pixel_format == "rgb24":
        check_height(H)
        px = np.asarray(frame).reshape(H, W, 3)
        return px[0::2], px[1::2]
    if pixel_format not in _yuv.FORMATS:
        raise ValueError(f"pixel_format: 'rgb24' or one of {_yuv.FORMATS}, got {pixel_format!r}")
    check_height(H, chroma == "420")
    flat = np.asarray(frame).reshape(-1)
    ch, cw = _yuv.chroma_shape(H, W, chroma)
    if flat.size != H * W + 2 * ch * cw:
        raise ValueError(f"expected {H * W + 2 * ch * cw} samples, got {flat.size}")
    y = flat[:H * W].reshape(H, W)
    c = flat[H * W:].reshape((ch, 2 * cw) if pixel_format == "nv12" else (2, ch, cw))
    out = []
    for p in (0, 1):
        cf = c[p::2] if pixel_format == "nv12" else c[:, p::2]
        out.append(np.concatenate([y[p::2].reshape(-1), cf.reshape(-1)]).reshape(-1, W))
    return out[0], out[1]


def decode_fields(frame, pixel_format: str, H: int, W: int, in_depth: int = 8, chroma="420", packing=None, matrix: str = "bt709",
                  full_range=False, siting="left") -> np.ndarray:
    """The woven RGB [H, W, 3] of a pushed frame (uint8, or uint16 in 0 .. 1023 at an input depth of 10 and for a 10-bit packing): each
    field decoded as a picture of H / 2 rows by yuv.to_rgb, depth10.to_rgb10, packed.to_rgb or, for RGB, taken as it is (values10 at 10
    bits)."""
    h = H // 2
    decoded = []
    for f in field_frames(frame, pixel_format, H, W, in_depth, chroma, packing):
        if packing not in (None, "none"):
            decoded.append(_packed.to_rgb(f, packing, h, W, matrix, full_range, siting))
        elif pixel_format == "rgb24":
            decoded.append(_d10.values10(f, "rgb10") if in_depth == 10 else f)
        elif in_depth == 10:
            decoded.append(_d10.to_rgb10(f, "p010" if pixel_format == "nv12" else "i010", h, W, matrix, full_range, siting, chroma))
        else:
            decoded.append(_yuv.to_rgb(f, pixel_format, h, W, matrix, full_range, siting, chroma))
    out = np.empty((H, W, 3), decoded[0].dtype)
    out[0::2], out[1::2] = decoded
    return out
