"""Inverse telecine: field matching and 1-in-5 decimation ahead of the streaming session's ring, stated once on the host (include/pfnl_hip.h
TELECINE; the kernels: csrc/telecine.hip; the index rules the session shares: csrc/telecine_geom.h).  numpy and Python integers only.

Film carried at 29.97 frames a second is 24 progressive frames a second spread over fields by 3:2 pulldown: film frames cover three and two
fields in turn, so of every five pushed frames two are woven from two different film frames and one repeats a picture.  The film frames
are all there, intact as field pairs: re-pairing the fields recovers them exactly, dropping the repeat restores the film's rate.

The vocabulary is pfnl_amd/deinterlace.py's: N pushed frames are the fields k = 0 .. 2 N - 1 in time order under ``field_order``; an index
past the ends is ``deinterlace.replace``d; every sample read is min(v, MAX), MAX = 255 | 1023; each of the 3 W samples of a row is handled
alone - the rule has no horizontal term.

MATCHING.  For pushed frame n the kept field is A = field 2 n, the first in time, of parity p.  Its partner is field 2 n + 1 (candidate
"c": the frame as pushed) or field 2 n - 1 (candidate "p"; at n = 0 that index is replaced and becomes field 1, so c = p there).  A film
frame covers two or three consecutive fields, so one of A's two neighbours in time always belongs to A's film frame: two candidates are
enough for a clean pulldown in any phase and either field order.

THE COMB COUNT of a candidate X.  Every missing row j = 0 .. h - 1 (h = H / 2), u = j - p, field rows clamped to [0, h - 1] as the
deinterlacer clamps them; for every sample of the row

    a = X[j] - A[u],  b = X[j] - A[u + 1];  the sample is combed iff a b > T^2

- the partner's sample lies on one side of both of its vertical neighbours by more than T.  T = ``threshold`` at 8 bits and 4 ``threshold``
at 10 bits.  The count is the number of combed samples: an exact integer, at most h 3 W.

THE CHOICE.  The candidate with the smaller count, "c" on a tie; the matched frame m_n is the weave of A and the chosen partner.  With
``post`` on, a frame whose smaller count exceeds ``comb_limit`` is video, not film: m_n is then deinterlace.frames(..., rate="frame")[n],
the existing rule at the time of field 2 n, byte for byte.

DEFAULTS.  threshold 10, post on, comb_limit (h 3 W) >> 8.  They are parameters of the rule - chosen, not measured.

DECIMATION (mode "decimate").  D_n = sum |m_n - m_(n-1)| over all samples; D_0 is the largest uint64.  Frames 5 q .. 5 q + 4, counted
from the start of the sequence, are cycle q.  Of a complete cycle the frame with the smallest D is dropped (the lowest index on a tie) and
the other four are delivered in order; an incomplete last cycle is delivered whole.  Mode "match" delivers every m_n.  A cut mark on a
pushed frame lands on the first delivered frame made from it, or from a later frame where its own is dropped (a mark behind the last
delivered frame is lost).  Cycles do not restart at marks: the rate stays 4 / 5 throughout.

LATENCY.  m_n exists once frame n + 1 has been pushed, or at the end - the deinterlacer's one frame, which ``post`` needs.  In mode
"decimate" a cycle's frames are admitted together when its last matched frame exists.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import deinterlace as _deint

MODES = ("match", "decimate")                                           # PFNL_TELECINE_MATCH, _DECIMATE are index + 1 (0: off)
CYCLE = 5                                                               # pushed frames per decimation cycle: one of them is dropped
THRESHOLD = 10                                                          # the defaults: parameters of the rule, chosen and not measured
POST = True
D_FIRST = (1 << 64) - 1                                                 # D_0: the first frame of a sequence is never the repeat


def mode_id(mode) -> int:
    """The C-ABI's PFNL_TELECINE_* value of ``mode``: None 0 (off), "match" 1, "decimate" 2; ValueError for anything else."""
    if mode is None:
        return 0
    if not isinstance(mode, str) or mode not in MODES:
        raise ValueError(f"telecine: None or one of {MODES}, got {mode!r}")
    return MODES.index(mode) + 1


def comb_limit_default(h: int, W: int) -> int:
    """(h 3 W) >> 8: one sample in 256 of a field"""
    return (int(h) * 3 * int(W)) >> 8


def params(h: int, W: int, threshold: Optional[int] = None, post: Optional[bool] = None, comb_limit: Optional[int] = None) -> Tuple[int, int, int]:
    """(threshold, post, comb_limit) with the defaults filled in, as pfnl_telecine_params carries them; ValueError outside
    1 <= threshold <= 255, comb_limit >= 0."""
    threshold = THRESHOLD if threshold is None else int(threshold)
    post = POST if post is None else bool(post)
    comb_limit = comb_limit_default(h, W) if comb_limit is None else int(comb_limit)
    if not 1 <= threshold <= 255:
        raise ValueError(f"telecine: threshold in 1 .. 255, got {threshold}")
    if comb_limit < 0:
        raise ValueError(f"telecine: comb_limit is not negative, got {comb_limit}")
    return threshold, int(post), comb_limit


def _clipped(a, maxv: int) -> np.ndarray:
    if maxv not in (255, 1023):
        raise ValueError(f"maxv: 255 or 1023, got {maxv!r}")
    a = np.asarray(a).astype(np.int64)
    if a.ndim < 1 or a.shape[0] < 1:
        raise ValueError("a field is [H / 2, ...]")
    if a.size and int(a.min()) < 0:
        raise ValueError("samples are not negative")
    return np.minimum(a, maxv)


def comb_count(A, X, parity: int, threshold: int = THRESHOLD, maxv: int = 255) -> int:
    """The comb count of the partner X beside the kept field A of parity ``parity``: both [H / 2, ...] of one shape."""
    if parity not in (0, 1):
        raise ValueError(f"parity: 0 or 1, got {parity!r}")
    A, X = _clipped(A, maxv), _clipped(X, maxv)
    if A.shape != X.shape:
        raise ValueError("the two fields have one shape, [H / 2, ...]")
    h = A.shape[0]
    T = int(threshold) * (1 if maxv == 255 else 4)
    u = np.arange(h) - parity
    a = X - A[np.clip(u, 0, h - 1)]
    b = X - A[np.clip(u + 1, 0, h - 1)]
    return int((a * b > T * T).sum())


def match(A, Xc, Xp, parity: int, threshold: int = THRESHOLD, maxv: int = 255) -> Tuple[str, int, int]:
    """("c" | "p", count of c, count of p): the candidate with the smaller count, "c" on a tie."""
    cc, cp = comb_count(A, Xc, parity, threshold, maxv), comb_count(A, Xp, parity, threshold, maxv)
    return ("p" if cp < cc else "c"), cc, cp


def weave(A, X, parity: int, maxv: int = 255) -> np.ndarray:
    """The frame [H, ...] whose rows parity, parity + 2, ... are A and whose other rows are X: uint8 for maxv 255, uint16 for 1023."""
    A, X = _clipped(A, maxv), _clipped(X, maxv)
    out = np.empty((2 * A.shape[0],) + A.shape[1:], np.uint8 if maxv == 255 else np.uint16)
    out[parity::2] = A
    out[1 - parity::2] = X
    return out


def match_fields(n: int, n_frames: int) -> Tuple[int, int, int]:
    """(A, c, p): the fields the match of pushed frame n of ``n_frames`` reads, after the replacement at the start."""
    if not 0 <= n < n_frames:
        raise ValueError(f"frame {n} of {n_frames}")
    return 2 * n, 2 * n + 1, _deint.replace(2 * n - 1, 2 * n_frames)


def matched_frames(rgb_frames: Sequence, field_order="tff", threshold: Optional[int] = None, post: Optional[bool] = None,
                   comb_limit: Optional[int] = None, maxv: int = 255) -> Tuple[List[np.ndarray], List[Dict[str, int]]]:
    """(m, decisions): the matched frames of N pushed frames [H, W, 3] and, per frame, {"match": 0 (c) | 1 (p), "post": 0 | 1, "count_c",
    "count_p"}."""
    seq = _deint.sequence_fields(rgb_frames, field_order)
    N = len(seq) // 2
    h, W = seq[0][0].shape[0], seq[0][0].shape[1]
    threshold, post, comb_limit = params(h, W, threshold, post, comb_limit)
    video = None
    out, decisions = [], []
    for n in range(N):
        ka, kc, kp = match_fields(n, N)
        A, parity = seq[ka]
        which, cc, cp = match(A, seq[kc][0], seq[kp][0], parity, threshold, maxv)
        flagged = bool(post) and min(cc, cp) > comb_limit
        if flagged:
            if video is None:
                video = _deint.frames(rgb_frames, field_order, "frame", maxv)
            out.append(video[n])
        else:
            out.append(weave(A, seq[kc if which == "c" else kp][0], parity, maxv))
        decisions.append({"match": int(which == "p"), "post": int(flagged), "count_c": cc, "count_p": cp})
    return out, decisions


def frame_distance(a, b) -> int:
    """D: sum |a - b| over all samples of two matched frames"""
    return int(np.abs(np.asarray(a).astype(np.int64) - np.asarray(b).astype(np.int64)).sum())


def distances(matched: Sequence) -> List[int]:
    return [D_FIRST if n == 0 else frame_distance(matched[n], matched[n - 1]) for n in range(len(matched))]


def drop_index(d: Sequence[int]) -> int:
    """the frame of a complete cycle that is dropped: the smallest D, the lowest index on a tie"""
    if len(d) != CYCLE:
        raise ValueError(f"a complete cycle has {CYCLE} frames")
    return min(range(CYCLE), key=lambda j: (int(d[j]), j))


def place_marks(marks: Sequence[bool], drop: Optional[int], carry: bool = False) -> Tuple[List[bool], bool]:
    """(the marks of the delivered frames of one cycle, the mark carried into the next cycle): ``marks`` are the cycle's pushed frames',
    ``drop`` the dropped index or None (an incomplete cycle), ``carry`` what the cycle before left."""
    out = []
    for j, m in enumerate(marks):
        carry = carry or bool(m)
        if j == drop:
            continue
        out.append(carry)
        carry = False
    return out, carry


def decimate(matched: Sequence, marks: Optional[Sequence[bool]] = None):
    """(delivered frames, dropped indices, marks of the delivered frames) of the matched frames of a whole sequence"""
    d = distances(matched)
    marks = [False] * len(matched) if marks is None else list(marks)
    out, dropped, out_marks, carry = [], [], [], False
    for q in range(0, len(matched), CYCLE):
        idx = list(range(q, min(q + CYCLE, len(matched))))
        drop = drop_index(d[q:q + CYCLE]) if len(idx) == CYCLE else None
        if drop is not None:
            dropped.append(q + drop)
        got, carry = place_marks([marks[i] for i in idx], drop, carry)
        out += [matched[i] for j, i in enumerate(idx) if j != drop]
        out_marks += got
    return out, dropped, out_marks


def deliverable(mode, pushed: int, ended: bool) -> int:
    """How many ring frames a session in ``mode`` has made of ``pushed`` pushed frames (pfnl_telecine_deliverable): matched frame n exists
    once frame n + 1 is pushed or the sequence has ended; "decimate" admits four frames per complete cycle and an incomplete cycle at
    the end."""
    matched = pushed if ended else max(pushed - 1, 0)
    if mode_id(mode) == 1:
        return matched
    return 4 * (matched // CYCLE) + (matched % CYCLE if ended else 0)


def frames(rgb_frames: Sequence, mode="decimate", field_order="tff", threshold: Optional[int] = None, post: Optional[bool] = None,
           comb_limit: Optional[int] = None, maxv: int = 255) -> List[np.ndarray]:
    """The whole rule on a sequence of N pushed frames [H, W, 3]: the frames a session in ``mode`` puts into its ring."""
    if mode_id(mode) == 0:
        raise ValueError(f"telecine: one of {MODES}, got {mode!r}")
    m, _ = matched_frames(rgb_frames, field_order, threshold, post, comb_limit, maxv)
    return m if mode == "match" else decimate(m)[0]


def stats(rgb_frames: Sequence, mode="decimate", field_order="tff", threshold: Optional[int] = None, post: Optional[bool] = None,
          comb_limit: Optional[int] = None, maxv: int = 255) -> Tuple[int, int, int, int, int]:
    """(matched c, matched p, post-processed, dropped, delivered) as pfnl_stream_telecine_stats reports them for the whole sequence: a
    post-processed frame counts there and under neither match."""
    m, dec = matched_frames(rgb_frames, field_order, threshold, post, comb_limit, maxv)
    dropped = len(decimate(m)[1]) if mode == "decimate" else 0
    flagged = sum(d["post"] for d in dec)
    p = sum(d["match"] and not d["post"] for d in dec)
    return len(m) - flagged - p, p, flagged, dropped, len(m) - dropped


# ---- the forward 3:2 telecine, so that tests and users can make material --------------------------------------------------------------------
CADENCE = (0, 0, 0, 1, 1, 2, 2, 2, 3, 3)                                # the film frame under each of the ten fields of a cadence of four


def pulldown_fields(n_film: int, phase: int, n_frames: Optional[int] = None) -> List[int]:
    """The film frame under each of the 2 N fields of a 3:2 stream that starts ``phase`` pushed frames into the cadence (0 .. 4).  A stream
    cannot start with half a film frame and give it back, so a lone first field is paired: with the two fields behind it (1 + 2 -> 3,
    phase 1) or with one of the three behind it (1 + 3 -> 2 + 2, phase 2).  The last film frame stands for everything behind it.
    N = ceil(5 n_film / 4) where ``n_frames`` is None."""
    if phase not in range(CYCLE):
        raise ValueError(f"phase: 0 .. {CYCLE - 1}, got {phase!r}")
    if n_film < 1:
        raise ValueError("a film has at least one frame")
    N = -(-CYCLE * n_film // 4) if n_frames is None else int(n_frames)
    raw = [4 * (t // 10) + CADENCE[t % 10] for t in range(2 * phase, 2 * phase + 2 * N + 3)]
    if raw[0] != raw[1]:
        if raw.count(raw[1]) == 2:
            raw[0] = raw[1]
        else:
            raw[1] = raw[0]
    return [min(v - raw[0], n_film - 1) for v in raw[:2 * N]]


def pulldown(film: Sequence, phase: int = 0, field_order="tff", n_frames: Optional[int] = None) -> List[np.ndarray]:
    """The pushed frames of the film frames [H, W, 3] (H even) under 3:2 pulldown: field k of the stream, of the parity ``field_order``
    gives it, is the rows of that parity of film frame pulldown_fields(...)[k]."""
    film = [np.asarray(f) for f in film]
    first = _deint.order_id(field_order)
    under = pulldown_fields(len(film), phase, n_frames)
    out = []
    for n in range(len(under) // 2):
        frame = np.empty_like(film[0])
        for k in (2 * n, 2 * n + 1):
            p = (k & 1) ^ first
            frame[p::2] = film[under[k]][p::2]
        out.append(frame)
    return out
