"""The streaming session stated once on the host (include/pfnl_hip.h pfnl_stream_*; pfnl_amd/csrc/capi_stream.hip): its settings as the
factors of a ``Row``, what the library refuses (``legal``), a deterministic pairwise covering array over the legal rows
(``covering_rows``), the frames a session with a row's settings must deliver (``expected``) and a driver on the C-ABI that can move an OPEN
session from one row to the next (``RawSession``).  tests/test_session_model_host.py checks the model where it can be checked without a
device; tests/test_gpu_session_pairs.py compares the library with it byte for byte.

``expected`` adds no arithmetic: it composes the host rules the repository already states - yuv / depth10 / packed for the two edges,
deinterlace ahead of the ring, fit / resize behind the quantisation - around ``base``, the plain progressive RGB session, which the tests of
the stream, the scenes, the ensemble and the tiles hold to the forward.  A delivered frame is a pure function of the bytes that session
delivers (include/pfnl_hip.h), so ``base`` is a callable: on the device a second engine with the same weights, on the host a stand-in.

Two settings have no setter: ``batch`` is an argument of pfnl_stream_open and the weights (``fence``) belong to the engine.  A live session
therefore walks the rows of one (fence, batch) - ``walk_keys`` - and the look-ahead of T / 2 = 3 frames means that three pushed frames
launch a batch only once pfnl_stream_end has been called: that is how ``RawSession.abandon`` leaves work in flight.
"""
from __future__ import annotations

import ctypes as C
import functools
import itertools
from collections import namedtuple

import numpy as np

from pfnl_amd import _capi, deinterlace, depth10, fit, packed, resize, stream, surface, yuv

H, W, SCALE, T = 16, 24, 4, 7                                            # the frame; the network delivers 64 x 96
SH, SW = SCALE * H, SCALE * W
F = 5                                                                    # pushed frames: the last batch of 2 and of 3 is partial
CUT = 3                                                                  # the pushed frame that starts the second scene
THRESHOLD = 10.0                                                         # the detector's (tests/test_gpu_scene.py)
TILING = (12, 16, 2, 3)                                                  # 2 x 2 tiles of 12 x 16 with a margin of 2, in runs of 3
FILL = (200, 30, 90)

_RGB_PACKINGS = {"bgr24": 8, "rgba": 8, "bgra": 8, "x2rgb10": 10, "x2bgr10": 10}
_YUV_PACKINGS = {"yuyv422": 8, "uyvy422": 8, "y210": 10, "v210": 10}

# in: (pixel_format, in_depth, chroma, packing)
IN_VALUES = (tuple(("rgb24", d, "420", None) for d in (8, 10))
             + tuple((f, d, c, None) for f in ("nv12", "i420") for d in (8, 10) for c in ("420", "422", "444"))
             + tuple(("rgb24", d, "420", p) for p, d in _RGB_PACKINGS.items())
             + tuple(("nv12", d, "422", p) for p, d in _YUV_PACKINGS.items()))
# out: (out_format, out_chroma, out_packing)
OUT_VALUES = ((("rgb24", "420", None), ("rgb10", "420", None))
              + tuple((f, c, None) for f in ("nv12", "i420", "p010", "i010") for c in ("420", "422", "444"))
              + tuple(("rgb24" if d == 8 else "rgb10", "420", p) for p, d in _RGB_PACKINGS.items())
              + tuple(("nv12" if d == 8 else "p010", "422", p) for p, d in _YUV_PACKINGS.items()))
# size: name -> the keywords of stream.placement_arguments; every width is a multiple of 6 but the odd one
SIZES = {
    "off": {},
    "shrink": {"out_size": (48, 72)},
    "grow": {"out_size": (80, 120)},
    "odd": {"out_size": (37, 55)},
    "contain": {"out_size": (64, 144), "fit": "contain"},
    "crop": {"crop": (8, 12, 40, 60)},
    "place": {"out_size": (72, 120), "crop": (4, 6, 48, 72), "place": (10, 18, 50, 84), "fill": FILL},
}
VALUES = {
    "in": IN_VALUES,
    "out": OUT_VALUES,
    "interlace": (None, ("frame", "tff"), ("frame", "bff"), ("field", "tff"), ("field", "bff")),
    "scenes": ("off", "manual", "detector"),
    "chroma_siting": yuv.SITINGS,
    "out_chroma_siting": yuv.SITINGS,
    "matrix": ("bt709", "bt601"),
    "full_range": (False, True),
    "size": tuple(SIZES),
    "ensemble": (1, 2, 8),
    "tiling": (None, TILING),
    "batch": (1, 2, 3),
    "fence": (False, True),
    "push": ("host", "device", "host planes", "device planes"),
    "pop": ("host", "device", "host surface", "device surface"),
}
FACTORS = tuple(VALUES)
Row = namedtuple("Row", [("in_" if f == "in" else f) for f in FACTORS])
Row.get = lambda self, factor: self[FACTORS.index(factor)]               # ("in" is no attribute name)
DEFAULT = Row(*(VALUES[f][0] for f in FACTORS))                          # every setting as pfnl_stream_open leaves it
OUTSIDE_BASE = ("in", "out", "interlace", "chroma_siting", "out_chroma_siting", "matrix", "full_range", "size")


def with_(row: Row, **changes) -> Row:
    """``row`` with some factors changed (``in_`` for "in")."""
    return row._replace(**changes)


def in_depth(row: Row) -> int:
    return row.in_[1]


def out_depth(row: Row) -> int:
    return 10 if row.out[0] in _capi.TEN_BIT_FORMATS else 8


# ---- b. what the library refuses ------------------------------------------------------------------------------------------------------------
def arguments(row: Row, h: int = H, w: int = W) -> dict:
    """The arguments of every setter for ``row`` on frames of h x w, from the validators VideoStream.__init__ runs before it touches the
    engine; ValueError for a row the library refuses."""
    pf, depth, chroma, pack = row.in_
    of, out_chroma, out_pack = row.out
    rate, order = row.interlace or (None, "tff")
    size = SIZES[row.size]
    a = {"depth": stream.depth_argument(depth),
         "interlace": stream.interlace_arguments(rate, order, h, pf, chroma, pack),
         "format": stream.format_arguments(pf, of, row.matrix, row.full_range),
         "chroma": stream.chroma_arguments(chroma, out_chroma),
         "siting": stream.siting_arguments(row.chroma_siting, row.out_chroma_siting),
         "ensemble": stream.ensemble_argument(row.ensemble)}
    oH, oW, src, dst, fill = stream.placement_arguments(size.get("out_size"), SCALE * h, SCALE * w, of, size.get("crop"), size.get("fit"),
                                                        size.get("place"), (1, 1), size.get("fill", (0, 0, 0)), out_chroma)
    a["place"] = (oH, oW, src, dst, fill)
    a["canvas"] = (oH, oW) if oH else (SCALE * h, SCALE * w)
    a["packing"] = stream.packing_arguments(pack, out_pack, pf, of, depth, chroma, out_chroma, w, a["canvas"][1])
    a["tiling"] = stream.tiling_argument(h, w, *row.tiling) if row.tiling else None
    a["scenes"] = {"off": (0, 0.0), "manual": (1, 0.0), "detector": (2, THRESHOLD)}[row.scenes]
    return a


@functools.lru_cache(maxsize=None)
def _legal(key) -> bool:
    try:
        arguments(with_(DEFAULT, **dict(zip(("in_", "out", "interlace", "size", "ensemble", "tiling"), key))))
    except ValueError:
        return False
    return True


def legal(row: Row) -> bool:
    """Would the library take this row?  Computed without a device.  (The factors the validators do not look at - how frames are pushed and
    popped, the batch, the weights - and those every value of which they take - sitings, matrix, range, scenes - refuse nothing.)"""
    for f in ("scenes", "chroma_siting", "out_chroma_siting", "matrix", "full_range", "batch", "fence", "push", "pop"):
        if row.get(f) not in VALUES[f]:
            return False
    return _legal((row.in_, row.out, row.interlace, row.size, row.ensemble, row.tiling))


# ---- c. the covering array ------------------------------------------------------------------------------------------------------------------
def legal_pairs() -> list:
    """Every ((factor i, value index), (factor j, value index)), i < j, that some legal row holds, in sorted order.  A pair is legal when
    the row with those two values and every other factor at its default is: the defaults (planar RGB24 both ways, no size) go with all."""
    out = []
    for i, j in itertools.combinations(range(len(FACTORS)), 2):
        for a, va in enumerate(VALUES[FACTORS[i]]):
            for b, vb in enumerate(VALUES[FACTORS[j]]):
                row = list(DEFAULT)
                row[i], row[j] = va, vb
                if legal(Row(*row)):
                    out.append(((i, a), (j, b)))
    return out


@functools.lru_cache(maxsize=None)
def covering_rows() -> tuple:
    """A constrained pairwise array: legal rows that between them hold every legal pair.  Greedy and deterministic - everything is iterated
    in the order of FACTORS and VALUES, ties go to the lowest index: a row starts from the first uncovered pair, and every other factor
    takes the legal value that covers most uncovered pairs with what the row holds already, then the one with most uncovered pairs left,
    then the values in turn."""
    n = len(FACTORS)
    uncovered = set(legal_pairs())
    left = {}                                                            # (factor, value) -> uncovered pairs it is part of
    for p, q in uncovered:
        left[p] = left.get(p, 0) + 1
        left[q] = left.get(q, 0) + 1
    rows = []
    while uncovered:
        (i, a), (j, b) = min(uncovered)
        held = {i: a, j: b}

        def as_row(extra=None):
            r = list(DEFAULT)
            for f, v in held.items():
                r[f] = VALUES[FACTORS[f]][v]
            if extra:
                r[extra[0]] = VALUES[FACTORS[extra[0]]][extra[1]]
            return Row(*r)

        for f in range(n):
            if f in held:
                continue
            best, best_score = None, None
            for v in range(len(VALUES[FACTORS[f]])):
                if not legal(as_row((f, v))):
                    continue
                new = sum(1 for g, u in held.items() if (((f, v), (g, u)) if f < g else ((g, u), (f, v))) in uncovered)
                score = (new, left.get((f, v), 0), v == (len(rows) + f) % len(VALUES[FACTORS[f]]))   # (nothing to gain: take turns)
                if best_score is None or score > best_score:
                    best, best_score = v, score
            held[f] = best
        row = as_row()
        assert legal(row)
        rows.append(row)
        for p in itertools.combinations(sorted(held.items()), 2):
            if p in uncovered:
                uncovered.discard(p)
                left[p[0]] -= 1
                left[p[1]] -= 1
    return tuple(rows)


def pairs_of(row: Row) -> set:
    idx = [(k, VALUES[f].index(row[k])) for k, f in enumerate(FACTORS)]
    return set(itertools.combinations(idx, 2))


def chunks(rows, size: int = 16) -> list:
    rows = list(rows)
    return [rows[k:k + size] for k in range(0, len(rows), size)]


def walk_keys(rows) -> dict:
    """(fence, batch) -> the rows a live session of that batch on an engine of those weights walks, in the order of ``rows``."""
    out = {}
    for r in rows:
        out.setdefault((r.fence, r.batch), []).append(r)
    return out


# ---- d. the frames a session must deliver ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def content(depth: int, h: int = H) -> tuple:
    """F RGB frames [H, W, 3] at the depth with a real cut ahead of frame CUT: one random image per scene and noise of +-2 (8-bit steps) a
    frame, as tests/test_gpu_scene.py makes its scenes."""
    rng = np.random.default_rng(5)
    maxv, step = (255, 1) if depth == 8 else (1023, 4)
    out = []
    for n in (CUT, F - CUT):
        base = rng.integers(0, maxv + 1, size=(h, W, 3))
        out += [np.clip(base + step * rng.integers(-2, 3, size=(h, W, 3)), 0, maxv).astype(np.uint8 if depth == 8 else np.uint16) for _ in range(n)]
    return tuple(out)


def _encode(rgb, fmt, chroma, pack, ten, matrix, full_range, siting):
    """An RGB frame at 8 or 10 bits in the layout of a side: the host rules' from_rgb."""
    if pack is not None:
        return packed.from_rgb(rgb, pack, matrix, full_range, siting)
    if fmt in ("rgb24", "rgb10"):
        return rgb
    if ten:
        return depth10.from_rgb10(rgb, {"nv12": "p010", "i420": "i010"}.get(fmt, fmt), matrix, full_range, siting, chroma)
    return yuv.from_rgb(rgb, fmt, matrix, full_range, siting, chroma)


@functools.lru_cache(maxsize=None)
def _pushed(in_, matrix, full_range, siting, h) -> tuple:
    pf, depth, chroma, pack = in_
    return tuple(np.ascontiguousarray(_encode(f, pf, chroma, pack, depth == 10, matrix, full_range, siting)) for f in content(depth, h))


def pushed_frames(row: Row, h: int = H) -> tuple:
    """The F frames pushed into a session of ``row``, in its input layout: ``content`` encoded with the row's matrix, range and siting."""
    return _pushed(row.in_, row.matrix, row.full_range, row.chroma_siting, h)


def decode(row: Row, frame, h: int = H):
    """The host rule's RGB of one pushed progressive frame."""
    pf, depth, chroma, pack = row.in_
    rest = (row.matrix, row.full_range, row.chroma_siting)
    if pack is not None:
        return packed.to_rgb(frame, pack, h, W, *rest)
    if pf == "rgb24":
        return depth10.values10(frame, "rgb10") if depth == 10 else np.asarray(frame)
    if depth == 10:
        return depth10.to_rgb10(frame, "p010" if pf == "nv12" else "i010", h, W, *rest, chroma)
    return yuv.to_rgb(frame, pf, h, W, *rest, chroma)


def ring_frames(row: Row, pushed, h: int = H) -> list:
    """The progressive RGB frames the ring receives: the decode of every pushed frame, or with interlacing on the deinterlacer's frames of
    their decoded fields."""
    if row.interlace is None:
        return [decode(row, f, h) for f in pushed]
    pf, depth, chroma, pack = row.in_
    rate, order = row.interlace
    woven = [deinterlace.decode_fields(f, pf, h, W, depth, chroma, pack, row.matrix, row.full_range, row.chroma_siting) for f in pushed]
    return deinterlace.frames(woven, order, rate, 255 if depth == 8 else 1023)


def marks(row: Row) -> tuple:
    """The ring frames a manual mark lands on: the first frame made from pushed frame CUT."""
    if row.scenes != "manual":
        return ()
    return (2 * CUT,) if row.interlace and row.interlace[0] == "field" else (CUT,)


def deliver(row: Row, rgb, h: int = H):
    """The output side on one frame of the plain session (uint8, or uint16 values 0 .. 1023 for a 10-bit output): the canvas, then the
    conversion, then the packing."""
    ten = out_depth(row) == 10
    oH, oW, src, dst, fill = arguments(row, h)["place"]
    if oH:
        if src is None:
            rgb = (depth10.resize10 if ten else resize.resize)(rgb, oH, oW)
        else:
            rgb = (depth10.place10 if ten else fit.place)(rgb, oH, oW, src, dst, fill)
    of, out_chroma, out_pack = row.out
    return np.ascontiguousarray(_encode(rgb, of, out_chroma, out_pack, ten, row.matrix, row.full_range, row.out_chroma_siting))


def base_row(row: Row) -> Row:
    """The plain progressive RGB session ``base`` is: planar RGB in at the row's input depth, planar RGB out at the row's output depth, and
    the row's scenes, ensemble, tiling, batch and weights."""
    return with_(DEFAULT, in_=("rgb24", in_depth(row), "420", None), out=("rgb10" if out_depth(row) == 10 else "rgb24", "420", None),
                 scenes=row.scenes, ensemble=row.ensemble, tiling=row.tiling, batch=row.batch, fence=row.fence)


def expected(row: Row, pushed, base, h: int = H) -> list:
    """[(index, frame)] a session of ``row`` delivers for ``pushed``.  ``base(base_row(row), rgb_frames, marks)`` -> the frames the plain
    session delivers for those ring frames: [sH, sW, 3] each, uint8 or uint16."""
    plain = base(base_row(row), ring_frames(row, pushed, h), marks(row))
    return [(i, deliver(row, f, h)) for i, f in enumerate(plain)]


def frame_layout(row: Row, h: int = H):
    """(shape, dtype) of a delivered frame: packed.frame_shape bytes with an output packing, else stream.frame_shapes samples."""
    of, out_chroma, out_pack = row.out
    oH, oW = arguments(row, h)["canvas"]
    if out_pack is not None:
        return packed.frame_shape(out_pack, oH, oW), np.dtype(np.uint8)
    return stream.frame_shapes(of, oH, oW, out_chroma)[0], np.dtype(stream.frame_dtype(of))


def standin_base(brow: Row, rgb_frames, marks_=()):
    """``base`` without a device: every ring frame repeated SCALE x SCALE and quantised at the output depth."""
    out = []
    for f in rgb_frames:
        v = np.asarray(f).astype(np.int64).repeat(SCALE, axis=0).repeat(SCALE, axis=1)
        top_in, top_out = (1 << in_depth(brow)) - 1, (1 << out_depth(brow)) - 1
        out.append(((2 * v * top_out + top_in) // (2 * top_in)).astype(np.uint16 if top_out == 1023 else np.uint8))
    return out


# ---- e. the driver --------------------------------------------------------------------------------------------------------------------------
PAD_FILL, PUSH_FILL = 0xA5, 0x3C
INVALID, STATE = -1, -2                                                  # PFNL_ERR_INVALID, PFNL_ERR_STATE


def in_planes(row: Row, frame, h: int = H) -> list:
    """The planes of a pushed frame as (rows, samples) arrays: the one plane of a packing's sample bytes, else surface.split."""
    pf, depth, chroma, pack = row.in_
    if pack is not None:
        return [np.asarray(frame).reshape(packed.frame_shape(pack, h, W))[:, :packed.row_bytes(pack, W)]]
    return surface.split(frame, stream.pushed_format(pf, depth), h, W, chroma)


def out_planes(row: Row, h: int = H) -> tuple:
    """((rows, row bytes), ...) of a delivered frame's planes."""
    of, out_chroma, out_pack = row.out
    oH, oW = arguments(row, h)["canvas"]
    return tuple((r, n * dt.itemsize) for r, n, dt in surface.plane_shapes(of, oH, oW, out_chroma, out_pack))


def _pitches(row_bytes) -> list:
    """20 bytes behind a row of the first plane, 10 behind one of the others (tests/test_gpu_input_route.py _pitched)."""
    return [n + (10 if k else 20) for k, n in enumerate(row_bytes)]


class RawSession:
    """One session on ``engine`` through ctypes alone: every setter can be called on it while it is open, which VideoStream cannot do."""

    def __init__(self, engine, batch: int, h: int = H):
        import torch
        self.torch = torch
        self.lib, self.engine, self.batch, self.h = engine._lib, engine, int(batch), int(h)
        cur = torch.cuda.current_stream(torch.device("cuda", engine.device)).cuda_stream
        s = C.c_void_p()
        self._ok(self.lib.pfnl_stream_open(engine._h, self.h, W, self.batch, C.c_void_p(cur) if cur else None, C.byref(s)), "open")
        self.s = s
        self.row = with_(DEFAULT, batch=self.batch)                      # what the session is set to
        self.keep = []                                                   # device frames of the running sequence
        self.cuts = []

    # -- plumbing
    def error(self) -> str:
        msg = self.lib.pfnl_last_error()
        return msg.decode() if msg else "?"

    def _ok(self, status, what):
        assert status == 0, f"{what}: status {status}: {self.error()}"

    def close(self):
        if self.s is not None:
            s, self.s = self.s, None
            self._ok(self.lib.pfnl_stream_close(s), "close")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def reset(self):
        self._ok(self.lib.pfnl_stream_reset(self.s), "reset")
        self.keep, self.cuts = [], []

    def end(self):
        st = self.lib.pfnl_stream_end(self.s)
        if st == STATE and "pop first" in self.error():
            return False
        self._ok(st, "end")
        return True

    def ready(self) -> int:
        n = C.c_int(0)
        self._ok(self.lib.pfnl_stream_ready(self.s, C.byref(n)), "ready")
        return n.value

    # -- the setting
    def calls(self, row: Row) -> list:
        """[(name, function, arguments)] that set ``row``, each setting's off value where the row has it off."""
        a = arguments(row, self.h)
        lib = self.lib
        oH, oW, src, dst, fill = a["place"]
        if src is None:
            size = ("resize", lib.pfnl_stream_resize, (oH, oW))
        else:
            size = ("place", lib.pfnl_stream_place, (oH, oW, _capi.rect_arg(src), _capi.rect_arg(dst), (C.c_uint8 * 3)(*fill)))
        tile = None if a["tiling"] is None else C.byref(_capi.pfnl_tiling(*a["tiling"]))
        return [("scenes", lib.pfnl_stream_scenes, a["scenes"]), ("input_depth", lib.pfnl_stream_input_depth, (a["depth"],)),
                ("format", lib.pfnl_stream_format, a["format"]), ("chroma_siting", lib.pfnl_stream_chroma_siting, a["siting"]),
                ("chroma_format", lib.pfnl_stream_chroma_format, a["chroma"]), size, ("packing", lib.pfnl_stream_packing, a["packing"]),
                ("ensemble", lib.pfnl_stream_ensemble, (a["ensemble"],)), ("interlace", lib.pfnl_stream_interlace, a["interlace"]),
                ("tile", lib.pfnl_stream_tile, (tile,))]

    def configure(self, row: Row) -> int:
        """From whatever the session is set to now to ``row``; returns the calls that were answered PFNL_ERR_INVALID and repeated."""
        assert row.batch == self.batch, "the batch is pfnl_stream_open's"
        if (self.row.in_[3], self.row.out[2]) != (row.in_[3], row.out[2]):   # "set PFNL_PACK_NONE first"
            self._ok(self.lib.pfnl_stream_packing(self.s, 0, 0), "packing(0, 0)")
        pending, repeated = self.calls(row), 0
        while pending:
            later = []
            for name, fn, args in pending:
                st = fn(self.s, *args)
                if st == INVALID:                                        # whichever comes second checks against the other's setting
                    later.append((name, fn, args, self.error()))
                else:
                    self._ok(st, name)
            assert len(later) < len(pending), "no call makes progress: " + "; ".join(f"{n}{a[:3]}: {why}" for n, _, a, why in later)
            repeated += len(later)
            pending = [c[:3] for c in later]
        self.row = row
        return repeated

    # -- frames in
    def _surface(self, bufs, pitches):
        ptr = [b.data_ptr() if hasattr(b, "data_ptr") else b.ctypes.data for b in bufs]
        pad = 3 - len(ptr)
        return _capi.pfnl_surface((C.c_void_p * 3)(*ptr, *([None] * pad)), (C.c_size_t * 3)(*pitches, *([0] * pad)))

    def _push_call(self, frame, way):
        frame = np.ascontiguousarray(frame)
        if way in ("host", "device"):
            buf = frame if way == "host" else self.torch.from_numpy(frame.reshape(-1).view(np.uint8)).cuda()
            self.keep.append(buf)
            ptr = buf.ctypes.data_as(C.c_void_p) if way == "host" else C.c_void_p(buf.data_ptr())
            return lambda: self.lib.pfnl_stream_push(self.s, ptr, int(way == "device"))
        planes = in_planes(self.row, frame, self.h)
        pitches = _pitches([p.shape[1] * p.dtype.itemsize for p in planes])
        assert all(v % 16 for v in pitches)
        bufs = surface.embed(planes, pitches, PUSH_FILL)
        if way == "device planes":
            bufs = [self.torch.from_numpy(b).cuda() for b in bufs]
        sf = self._surface(bufs, pitches)
        self.keep.append((bufs, sf))
        return lambda: self.lib.pfnl_stream_push_surface(self.s, C.byref(sf), int(way == "device planes"))

    def push(self, frame, way, pop_way="host") -> list:
        """Hands one frame over; an interlaced session may ask for the ready frames first ("pop first": it has changed nothing) - they are
        popped, returned, and the push is repeated."""
        call = self._push_call(frame, way)
        st, got = call(), []
        if st == STATE and "pop first" in self.error():
            got = self.pop_all(pop_way)
            st = call()
        self._ok(st, f"push ({way})")
        return got

    def mark_cut(self):
        self._ok(self.lib.pfnl_stream_mark_cut(self.s), "mark_cut")

    # -- frames out
    def pop(self, way):
        """(index, frame) with the frame on the host in ``frame_layout``, or None.  Every buffer is pre-filled; a surface's bytes between a
        row's end and its pitch, and a tight frame's behind the frame, must still hold the fill."""
        row, torch = self.row, self.torch
        shape, dtype = frame_layout(row, self.h)
        planes = out_planes(row, self.h)
        index, got = C.c_longlong(0), C.c_int(0)
        device = way.startswith("device")
        if way in ("host", "device"):
            nbytes = int(np.prod(shape)) * dtype.itemsize
            buf = np.full(nbytes + 64, PAD_FILL, np.uint8)
            if device:
                buf = torch.from_numpy(buf).cuda()
            ptr = C.c_void_p(buf.data_ptr()) if device else buf.ctypes.data_as(C.c_void_p)
            self._ok(self.lib.pfnl_stream_pop(self.s, ptr, int(device), C.byref(index), C.byref(got)), f"pop ({way})")
            raw = buf.cpu().numpy() if device else buf
            assert (raw[nbytes:] == PAD_FILL).all(), f"pop ({way}) wrote behind the frame"
            if not got.value:
                assert (raw == PAD_FILL).all(), "a pop that delivers nothing writes nothing"
                return None
            frame = raw[:nbytes].view(dtype).reshape(shape)
        else:
            pitches = _pitches([n for _, n in planes])
            bufs = [np.full((rows + 1, pitch), PAD_FILL, np.uint8) for (rows, _), pitch in zip(planes, pitches)]   # (a row behind the last)
            if device:
                bufs = [torch.from_numpy(b).cuda() for b in bufs]
            sf = self._surface(bufs, pitches)
            self._ok(self.lib.pfnl_stream_pop_surface(self.s, C.byref(sf), int(device), C.byref(index), C.byref(got)), f"pop_surface ({way})")
            raw = [b.cpu().numpy() for b in bufs] if device else bufs
            for k, (b, (rows, n)) in enumerate(zip(raw, planes)):
                assert (b[:rows, n:] == PAD_FILL).all() and (b[rows:] == PAD_FILL).all(), f"pop_surface ({way}) wrote outside plane {k}'s samples"
            if not got.value:
                assert all((b == PAD_FILL).all() for b in raw), "a pop that delivers nothing writes nothing"
                return None
            if row.out[2] is not None:                                   # the tight frame's rows may be longer than their samples (v210): zeros
                frame = np.zeros(shape, np.uint8)
                frame[:, :planes[0][1]] = raw[0][:planes[0][0], :planes[0][1]]
            else:
                flat = np.concatenate([b[:rows, :n].reshape(-1) for b, (rows, n) in zip(raw, planes)])
                frame = flat.view(dtype).reshape(shape)
        if row.scenes != "off":
            first, sad = C.c_longlong(0), C.c_ulonglong(0)
            self._ok(self.lib.pfnl_stream_pop_info(self.s, C.byref(first), C.byref(sad)), "pop_info")
            if index.value > 0 and first.value == index.value:
                self.cuts.append(index.value)
        return index.value, np.array(frame)

    def pop_all(self, way) -> list:
        out = []
        for _ in range(self.ready()):
            item = self.pop(way)
            assert item is not None
            out.append(item)
        return out

    # -- sequences
    def run(self, pushed, mark_at=None) -> list:
        """A whole sequence the row's way: push, pop what is ready, ... end, pop the rest; then the session is reset."""
        row, got = self.row, []
        for i, f in enumerate(pushed):
            if mark_at is not None and i == mark_at:
                self.mark_cut()
            got += self.push(f, row.push, row.pop)
            got += self.pop_all(row.pop)
        if not self.end():
            got += self.pop_all(row.pop)
            assert self.end()
        got += self.pop_all(row.pop)
        assert self.pop(row.pop) is None
        cuts = list(self.cuts)
        self.reset()
        return got, cuts

    def abandon(self, pushed):
        """Leaves work in flight: three frames, the last through a device pointer, the end (with a look-ahead of T / 2 = 3 frames that is
        what launches their batches), no pop."""
        row = self.row
        for i, f in enumerate(pushed[:3]):
            self.push(f, row.push if i < 2 else ("device planes" if "planes" in row.push else "device"), row.pop)
        self.end()
        assert self.ready() > 0
