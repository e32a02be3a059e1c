"""VideoStream - the Python face of the C-ABI's streaming session (include/pfnl_hip.h, pfnl_stream_*).

uint8 LR frames go in one at a time, uint8 SR frames come out in order; the clamped windows, the batching, the quantisation and the
range-flag recovery of the harness (pfnl_amd/model.py _run_sequence_on_device; reference model/pfnl.py:236-262) happen inside the
library.  Nothing here computes::

    with model.open_stream(H, W, batch=4) as vs:
        for frame in decoder:                      # [H,W,3] uint8
            for index, sr in vs.push(frame):       # [] until a batch of 4 has its look-ahead of T/2 frames
                sink(index, sr)                    # [sH,sW,3] uint8
        for index, sr in vs.end():
            sink(index, sr)

Scenes (off by default): ``open_stream(H, W, batch, scene_cut=10.0)`` runs the cut detector of pfnl_amd/scene.py on the device ring, and
``scene_cut="manual"`` takes the cuts from the caller (``vs.mark_cut()`` before the push of a scene's first frame); the windows of a frame
then stay inside its scene, and ``vs.cuts`` lists the delivered frames that started one.

YUV 4:2:0 (off by default): ``open_stream(H, W, batch, pixel_format="nv12")`` takes frames as a decoder delivers them - ``(H*3//2, W)``
uint8, or flat - and returns SR frames ``(sH*3//2, sW)`` for an encoder; ``"i420"`` likewise; ``out_format`` sets the two sides apart
(``"rgb24"`` among them).  The conversion runs on the device at the two edges of the session, by the integer rule of pfnl_amd/yuv.py
(``matrix`` "bt601" | "bt709", ``full_range``; chroma sited left, or where ``chroma_siting`` / ``out_chroma_siting`` say: "center" is what
JPEG and a Y4M stream's default ``C420jpeg`` mean, "topleft" UHD HEVC and ``C420paldv``); the ring, the scenes and the windows go on seeing RGB.

4:2:2 and 4:4:4 (off by default): ``open_stream(H, W, batch, pixel_format="i420", chroma="422")`` takes and delivers the layout at that
subsampling (pfnl_amd/yuv.py CHROMAS) - "i420" is then I422 / I444, "nv12" NV16 / NV24, and with ``in_depth=10`` / a 10-bit ``out_format``
yuv422p10le / yuv444p10le, P210 / P410: frames of ``(2*H, W)`` / ``(3*H, W)`` samples, or flat.  ``out_chroma`` sets the output side apart
(None = the input's).  An axis that is not subsampled takes no filter; the output size is even along the axes that are.

Output size (off by default): ``open_stream(H, W, batch, out_size=(1080, 1920))`` delivers every frame at that raster - ``(oH, oW, 3)``, or
``(oH*3//2, oW)`` in a 4:2:0 output format (then both even) - resampled on the device behind the quantisation and ahead of the YUV conversion by
the integer rule of pfnl_amd/resize.py (a Keys cubic that widens when the raster shrinks): each axis between a quarter and twice the
network's own size.

10 bits out (off by default): ``open_stream(H, W, batch, out_format="p010")`` delivers uint16 frames for an HEVC Main10 / AV1 encoder -
``(oH*3//2, oW)``, every sample value << 6; ``"i010"`` (yuv420p10le) the values themselves, ``"rgb10"`` ``(oH, oW, 3)`` with values 0 .. 1023:
the fp32 result quantised to 1023 levels instead of 255, then the same resampling and conversion by the rule of pfnl_amd/depth10.py.
These are names of output formats (``pixel_format`` stays "rgb24" | "nv12" | "i420"), and "rgb10" goes with RGB input.

10 bits in (off by default): ``open_stream(H, W, batch, pixel_format="i420", in_depth=10)`` takes uint16 frames in ``pixel_format``'s layout
at 10 bits - "i420" is then yuv420p10le (the values themselves), "nv12" P010 (the value in the upper ten bits), "rgb24" ``(H, W, 3)`` values
0 .. 1023: the conventions of the three 10-bit output formats.  The ring on the device holds uint16 samples, the network sees
value / 1023, scenes score luma on the 8-bit scale (pfnl_amd/depth10.py, pfnl_amd/scene.py luma_u10); everything behind the windows is
what it was, and with ``out_format="p010"`` the session is 10-bit end to end.

Placement (off by default): ``open_stream(H, W, batch, out_size=(1080, 1920), fit="contain")`` keeps the picture's aspect ratio - a 4:3
source lands 1080 x 1440 in the middle of a 16:9 canvas, bars of ``fill`` left and right; ``fit="cover"`` fills the canvas and loses two
edges; ``sar=(16, 15)`` honours non-square pixels; ``crop=(y, x, h, w)`` (SR-raster pixels) cuts bars off before the picture is scaled;
``place=(y, x, h, w)`` names the destination outright (``out_size=(1088, 1920), place=(0, 0, 1080, 1920)``: coded height, no resampling).
One launch on the device writes the canvas, by the integer rule of pfnl_amd/fit.py.

Packed formats (off by default): ``open_stream(H, W, batch, pixel_format="nv12", chroma="422", packing="yuyv422", out_format="rgb24",
out_packing="bgra")`` takes a capture card's frames and delivers a swap chain's: one plane of interleaved samples per frame
(pfnl_amd/packed.py PACKINGS - bgr24, rgba, bgra, yuyv422, uyvy422, x2rgb10, x2bgr10, y210, v210).  The two sides are independent and None
means planes; a packing goes with the family, depth and chroma format its side is set to (a YUV ``pixel_format`` only says the side is
YUV).  Frames are uint8 arrays of ``packed.frame_shape`` - bytes, whatever the unit - or flat.

Interlaced input (off by default): ``open_stream(H, W, batch, pixel_format="i420", interlaced="field", field_order="tff")`` takes WOVEN
frames - both fields in the pushed layout, whatever it is - and deinterlaces them on the device ahead of the ring by the integer rule of
pfnl_amd/deinterlace.py: one progressive frame per pushed frame at "frame", two at "field", a frame later than the push that brought
them.  Everything behind the ring is what it was.

Film under 3:2 pulldown (off by default): ``open_stream(H, W, batch, telecine="decimate", field_order="tff")`` takes the frames of film
carried at 29.97 frames a second, re-pairs their fields on the device ahead of the ring by the integer rule of pfnl_amd/telecine.py and drops
the one frame in five that repeats a picture: indices count film frames, and a cycle's four frames come together (``batch`` at least 2).
``telecine="match"`` keeps every frame.  Exclusive with ``interlaced``.

Colour per side (off by default): ``open_stream(480, 720, batch, pixel_format="i420", matrix="bt601", primaries="bt601-525",
out_size=(1080, 1440), out_matrix="bt709", out_primaries="bt709")`` takes a DVD's frames as they are and delivers what an HD stream is
read as: the input's matrix on the way in, the output's on the way out, and the primaries converted on the device in linear light by the
integer rule of pfnl_amd/colour.py, in the launch that quantises the SR frames.

Surfaces: ``vs.push_planes(y, cbcr)`` / ``vs.pop_planes(y, cbcr)`` take and fill a frame as a decoder or encoder holds it - one array per
plane, each with the row pitch its strides say (pfnl_amd/surface.py), e.g. ``surface[:H, :W]`` of a pitched device allocation - in the
session's formats; a device NV12 / I420 surface is converted where it lies, and only the samples of a destination are written.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Tuple

import numpy as np

from . import _capi, ensemble as _ensemble, fit as _fit, resize as _resize, surface as _surface, tiles as _tiles


def next_batch(num_frames: int, batch: int, pushed: int, ended: bool, launched: int) -> Tuple[int, int]:
    """(first, count) of the batch that may launch now, count = 0 for none (pfnl_stream_next_batch: the session's own rule; needs no
    device).  A sequence of F frames always runs as the batches [k*batch, min((k+1)*batch, F))."""
    first, count = C.c_longlong(0), C.c_int(0)
    _capi.check(_capi.load_library().pfnl_stream_next_batch(int(num_frames), int(batch), int(pushed), 1 if ended else 0, int(launched),
                                                            C.byref(first), C.byref(count)))
    return first.value, count.value


def format_arguments(pixel_format="rgb24", out_format=None, matrix="bt709", full_range=False) -> Tuple[int, int, int, int]:
    """The four arguments of pfnl_stream_format for open_stream's keywords (``out_format`` None = ``pixel_format``); ValueError for
    anything the library would refuse.  Needs no device."""
    if out_format is None:
        out_format = pixel_format
    for name, value in (("pixel_format", pixel_format), ("out_format", out_format)):
        if value not in _capi.PIXEL_FORMATS:
            raise ValueError(f"{name}: one of {sorted(_capi.PIXEL_FORMATS)}, got {value!r}")
    if pixel_format in _capi.TEN_BIT_FORMATS:
        raise ValueError(f"pixel_format: 10-bit input is in_depth=10 ({pixel_format!r} names an out_format; pixel_format names the layout), "
                         f"one of 'rgb24', 'nv12', 'i420'")
    if out_format == "rgb10" and pixel_format != "rgb24":
        raise ValueError(f"out_format 'rgb10' goes with pixel_format 'rgb24', got {pixel_format!r}")
    if matrix not in _capi.YUV_MATRICES:
        raise ValueError(f"matrix: one of {sorted(_capi.YUV_MATRICES)}, got {matrix!r}")
    if full_range not in (False, True, 0, 1):
        raise ValueError(f"full_range: False or True, got {full_range!r}")
    return _capi.PIXEL_FORMATS[pixel_format], _capi.PIXEL_FORMATS[out_format], _capi.YUV_MATRICES[matrix], int(bool(full_range))


def colour_arguments(matrix="bt709", full_range=False, out_matrix=None, out_full_range=None, primaries="bt709", out_primaries=None):
    """The two sides of pfnl_stream_colour for open_stream's keywords as ``((matrix, full_range, primaries), (...))`` of C-ABI values
    (``out_matrix`` / ``out_full_range`` / ``out_primaries`` None = the input's), or None - no call, the session as it always was - with the
    three ``out_`` keywords None and ``primaries`` "bt709"; ValueError for anything the library would refuse.  Needs no device."""
    from . import colour as _colour
    for name, value in (("matrix", matrix), ("out_matrix", out_matrix)):
        if not (value is None and name == "out_matrix") and (not isinstance(value, str) or value not in _capi.YUV_MATRICES):
            raise ValueError(f"{name}: one of {sorted(_capi.YUV_MATRICES)}, got {value!r}")
    for name, value in (("full_range", full_range), ("out_full_range", out_full_range)):
        if not (value is None and name == "out_full_range") and value not in (False, True, 0, 1):
            raise ValueError(f"{name}: False or True, got {value!r}")
    for name, value in (("primaries", primaries), ("out_primaries", out_primaries)):
        if not (value is None and name == "out_primaries") and (not isinstance(value, str) or value not in _colour.PRIMARIES):
            raise ValueError(f"{name}: one of {_colour.PRIMARIES}, got {value!r}")
    if out_matrix is None and out_full_range is None and out_primaries is None and primaries == "bt709":
        return None
    side = (_capi.YUV_MATRICES[matrix], int(bool(full_range)), _colour.primaries_id(primaries))
    return side, (side[0] if out_matrix is None else _capi.YUV_MATRICES[out_matrix], side[1] if out_full_range is None else int(bool(out_full_range)),
                  side[2] if out_primaries is None else _colour.primaries_id(out_primaries))


IN_LAYOUTS = {"rgb24": "rgb10", "nv12": "p010", "i420": "i010"}         # what pixel_format's layout is called at an input depth of 10


def depth_argument(in_depth=8) -> int:
    """The argument of pfnl_stream_input_depth for open_stream's ``in_depth``: 8 (off: no call) or 10; ValueError for anything else.
    Needs no device."""
    if isinstance(in_depth, bool) or in_depth not in (8, 10):
        raise ValueError(f"in_depth: 8 or 10, got {in_depth!r}")
    return int(in_depth)


def pushed_format(pixel_format: str, in_depth: int = 8) -> str:
    """The format name whose layout and sample type a pushed frame has: ``pixel_format`` itself at 8 bits, its 10-bit twin at 10."""
    return IN_LAYOUTS[pixel_format] if depth_argument(in_depth) == 10 else pixel_format


def frame_argument(frame, pixel_format: str, H: int, W: int, in_depth: int = 8, chroma: str = "420"):
    """``frame`` as ``push`` hands it on - a contiguous numpy array, or a contiguous tensor where it was one - after the checks that need
    no session: uint8 samples, uint16 at an input depth of 10, in one of ``frame_shapes``; ValueError otherwise."""
    layout = pushed_format(pixel_format, in_depth)
    shapes = frame_shapes(layout, H, W, chroma)
    name = np.dtype(frame_dtype(layout)).name
    if type(frame).__module__.startswith("torch"):
        if str(frame.dtype) != "torch." + name or tuple(frame.shape) not in shapes:
            raise ValueError(f"expected a {name} frame of shape {' or '.join(map(str, shapes))}, got {frame.dtype} {tuple(frame.shape)}")
        return frame.contiguous()
    frame = np.asarray(frame)
    if frame.dtype != np.dtype(name) or frame.shape not in shapes:
        raise ValueError(f"expected a {name} frame of shape {' or '.join(map(str, shapes))}, got {frame.dtype} {frame.shape}")
    return np.ascontiguousarray(frame)


def packed_frame_argument(frame, packing: str, H: int, W: int):
    """``frame`` as ``push`` hands it on with an input packing: a contiguous uint8 numpy array or tensor of ``packed.frame_shape``, or flat
    with the frame's bytes; ValueError otherwise."""
    from . import packed as _packed
    shapes = (_packed.frame_shape(packing, H, W), (_packed.frame_bytes(packing, H, W),))
    if type(frame).__module__.startswith("torch"):
        if str(frame.dtype) != "torch.uint8" or tuple(frame.shape) not in shapes:
            raise ValueError(f"expected a uint8 {packing} frame of shape {' or '.join(map(str, shapes))}, got {frame.dtype} {tuple(frame.shape)}")
        return frame.contiguous()
    frame = np.asarray(frame)
    if frame.dtype != np.uint8 or frame.shape not in shapes:
        raise ValueError(f"expected a uint8 {packing} frame of shape {' or '.join(map(str, shapes))}, got {frame.dtype} {frame.shape}")
    return np.ascontiguousarray(frame)


def siting_arguments(chroma_siting="left", out_chroma_siting=None) -> Tuple[int, int]:
    """The two arguments of pfnl_stream_chroma_siting for open_stream's keywords (``out_chroma_siting`` None = ``chroma_siting``);
    ValueError for anything the library would refuse.  Needs no device."""
    if out_chroma_siting is None:
        out_chroma_siting = chroma_siting
    for name, value in (("chroma_siting", chroma_siting), ("out_chroma_siting", out_chroma_siting)):
        if not isinstance(value, str) or value not in _capi.CHROMA_SITINGS:
            raise ValueError(f"{name}: one of {sorted(_capi.CHROMA_SITINGS)}, got {value!r}")
    return _capi.CHROMA_SITINGS[chroma_siting], _capi.CHROMA_SITINGS[out_chroma_siting]


def chroma_arguments(chroma="420", out_chroma=None) -> Tuple[int, int]:
    """The two arguments of pfnl_stream_chroma_format for open_stream's keywords (``out_chroma`` None = ``chroma``); ValueError for
    anything the library would refuse.  Needs no device."""
    if out_chroma is None:
        out_chroma = chroma
    for name, value in (("chroma", chroma), ("out_chroma", out_chroma)):
        if not isinstance(value, str) or value not in _capi.CHROMA_FORMATS:
            raise ValueError(f"{name}: one of {sorted(_capi.CHROMA_FORMATS)}, got {value!r}")
    return _capi.CHROMA_FORMATS[chroma], _capi.CHROMA_FORMATS[out_chroma]


def packing_arguments(packing=None, out_packing=None, pixel_format="rgb24", out_format=None, in_depth=8, chroma="420", out_chroma=None,
                      W: int = 2, out_W: int = 2) -> Tuple[int, int]:
    """The two arguments of pfnl_stream_packing for open_stream's ``packing`` / ``out_packing`` (None = planes; the sides are independent)
    on sides set by the other keywords, W pixels wide in and out_W out; ValueError with the table's words (pfnl_amd/packed.py
    side_refused) for a side that disagrees.  Needs no device."""
    from . import packed as _packed
    out_format = pixel_format if out_format is None else out_format
    out_chroma = chroma if out_chroma is None else out_chroma
    ids = []
    for key, name, fmt, depth, sub, w in (("packing", packing, pixel_format, depth_argument(in_depth), chroma, W),
                                          ("out_packing", out_packing, out_format, 10 if out_format in _capi.TEN_BIT_FORMATS else 8, out_chroma, out_W)):
        if name is not None and not isinstance(name, str):
            raise ValueError(f"{key}: None or one of {_packed.PACKINGS[1:]}, got {name!r}")
        ids.append(_packed.packing_id(name))
        why = _packed.side_refused(name, fmt in _capi.FORMATS_420, depth, sub, int(w))
        if why:
            raise ValueError(f"{key}: {why}")
    return ids[0], ids[1]


def interlace_arguments(interlaced=None, field_order="tff", H: int = 4, pixel_format="rgb24", chroma="420", packing=None) -> Tuple[int, int]:
    """The two arguments of pfnl_stream_interlace for open_stream's ``interlaced`` (None = off: no call) and ``field_order``, for frames of H
    rows in the input setting of the other keywords; ValueError for anything the library would refuse (pfnl_amd/deinterlace.py).  Needs no
    device."""
    from . import deinterlace as _deinterlace
    mode, order = _deinterlace.mode_id(interlaced), _deinterlace.order_id(field_order)
    if mode:
        _deinterlace.check_height(int(H), pixel_format in _capi.FORMATS_420 and chroma == "420" and packing in (None, "none"))
    return mode, order


def telecine_arguments(telecine=None, field_order="tff", telecine_params=None, H: int = 4, W: int = 2, pixel_format="rgb24", chroma="420",
                       packing=None, interlaced=None):
    """(mode, field order, (threshold, post, comb_limit)) of pfnl_stream_telecine for open_stream's ``telecine`` (None = off: no call),
    ``field_order`` and ``telecine_params`` (None, or a dict with any of "threshold", "post", "comb_limit"), for frames of H x W in the input
    setting of the other keywords; ValueError for anything the library would refuse (pfnl_amd/telecine.py).  Needs no device."""
    from . import deinterlace as _deinterlace, telecine as _telecine
    mode, order = _telecine.mode_id(telecine), _deinterlace.order_id(field_order)
    par = dict(telecine_params or {})
    if set(par) - {"threshold", "post", "comb_limit"}:
        raise ValueError(f"telecine_params: threshold, post, comb_limit; got {sorted(par)}")
    if mode:
        if interlaced is not None:
            raise ValueError("telecine and interlaced are exclusive: film carried in fields is matched, video is deinterlaced")
        _deinterlace.check_height(int(H), pixel_format in _capi.FORMATS_420 and chroma == "420" and packing in (None, "none"))
    return mode, order, _telecine.params(max(int(H) // 2, 1), int(W), par.get("threshold"), par.get("post"), par.get("comb_limit"))


def bars_argument(bars=None, H: int = 2, W: int = 2):
    """The limit of pfnl_stream_bars for open_stream's ``bars`` (None = off: no call), for frames of H x W; ValueError for anything the
    library would refuse (pfnl_amd/bars.py).  Needs no device."""
    from . import bars as _bars
    if bars is None:
        return None
    limit = _bars.check_limit(bars)
    if int(H) > _bars.MAX_SIDE or int(W) > _bars.MAX_SIDE:
        raise ValueError(f"bars: H and W are at most {_bars.MAX_SIDE}")
    return limit


class PopInfo(tuple):
    """``last_info`` of a session with ``bars``: the tuple ``(scene_first, sad)`` it always was, and ``info["box"]`` - the content box
    (y0, x0, h, w) of the frame - beside ``info["scene_first"]`` and ``info["sad"]``."""

    def __new__(cls, scene_first, sad, box):
        self = super().__new__(cls, (scene_first, sad))
        self.box = tuple(box)
        return self

    def __getitem__(self, key):
        if isinstance(key, str):
            if key not in ("scene_first", "sad", "box"):
                raise KeyError(key)
            return self.box if key == "box" else tuple.__getitem__(self, ("scene_first", "sad").index(key))
        return tuple.__getitem__(self, key)


def output_grid(out_format: str, out_chroma: str = "420") -> Tuple[int, int]:
    """(gy, gx): what the delivered size is a multiple of per axis - 2 along the axes a YUV ``out_format`` subsamples, else 1."""
    chroma_arguments(out_chroma)
    if out_format not in _capi.FORMATS_420:
        return 1, 1
    return {"420": (2, 2), "422": (1, 2), "444": (1, 1)}[out_chroma]


def resize_arguments(out_size, sH: int, sW: int, out_format: str = "rgb24", out_chroma: str = "420") -> Tuple[int, int]:
    """The two arguments of pfnl_stream_resize for open_stream's ``out_size`` (None = off = (0, 0)) behind a network output of sH x sW;
    ValueError for anything the library would refuse.  Needs no device."""
    if out_size is None:
        return 0, 0
    try:
        oH, oW = (int(v) for v in out_size)
    except (TypeError, ValueError):
        raise ValueError(f"out_size: None or (oH, oW), got {out_size!r}") from None
    _resize.check_limits(sH, oH)
    _resize.check_limits(sW, oW)
    gy, gx = output_grid(out_format, out_chroma)
    if oH % gy or oW % gx:
        raise ValueError(f"out_size: a {out_format} output needs even sizes, got {oH} x {oW}" if (gy, gx) == (2, 2) else
                         f"out_size: a 4:2:2 {out_format} output needs an even width, got {oH} x {oW}")
    return oH, oW


def placement_arguments(out_size, sH: int, sW: int, out_format: str = "rgb24", crop=None, fit=None, place=None, sar=(1, 1), fill=(0, 0, 0),
                        out_chroma: str = "420"):
    """``(oH, oW, src, dst, fill)`` for open_stream's ``out_size``, ``crop``, ``fit``, ``place``, ``sar`` and ``fill`` behind a network output
    of sH x sW: the arguments of pfnl_stream_place, rectangles as (y, x, h, w).  With ``crop``, ``fit`` and ``place`` at their defaults src and
    dst are None and (oH, oW) is resize_arguments' answer - pfnl_stream_resize, or no call at all for (0, 0).  The canvas is ``out_size``, else
    the crop's own size, else the network's raster.  ValueError for anything the library would refuse.  Needs no device."""
    fill = _fit.as_fill(fill)
    if fit not in (None, "contain", "cover"):
        raise ValueError(f'fit: None, "contain" or "cover", got {fit!r}')
    if fit is not None and place is not None:
        raise ValueError("fit and place exclude each other: place names the destination that fit would work out")
    try:
        sar = tuple(int(v) for v in sar)
    except (TypeError, ValueError):
        raise ValueError(f"sar: (num, den), got {sar!r}") from None
    if len(sar) != 2 or sar[0] < 1 or sar[1] < 1:
        raise ValueError(f"sar: two positive integers, got {sar!r}")
    if sar[0] != sar[1] and fit is None:
        raise ValueError('sar goes with fit="contain" or "cover"')
    oH, oW = resize_arguments(out_size, sH, sW, out_format, out_chroma) if crop is None and fit is None and place is None else (0, 0)
    if crop is None and fit is None and place is None:
        return oH, oW, None, None, fill
    src = _fit.as_rect(crop, "crop", sH, sW)
    if out_size is None:
        oH, oW = (src[2], src[3]) if crop is not None else (sH, sW)
    else:
        try:
            oH, oW = (int(v) for v in out_size)
        except (TypeError, ValueError):
            raise ValueError(f"out_size: None or (oH, oW), got {out_size!r}") from None
    g = output_grid(out_format, out_chroma)
    if oH % g[0] or oW % g[1]:
        raise ValueError(f"a {out_format} output needs an even canvas, got {oH} x {oW}" if g == (2, 2) else
                         f"a 4:2:2 {out_format} output needs a canvas of even width, got {oH} x {oW}")
    g = g[0] if g[0] == g[1] else g
    if place is not None:
        dst = _fit.as_rect(place, "place", oH, oW)
        _fit.check_rects(sH, sW, oH, oW, src, dst)
    else:
        src, dst = _fit.rects(sH, sW, oH, oW, crop, fit, sar, g)
    return oH, oW, src, dst, fill


def ensemble_argument(ensemble=1) -> int:
    """The argument of pfnl_stream_ensemble for open_stream's ``ensemble``: 1 (off: no call), 2, 4 or 8 members of pfnl_amd/ensemble.py;
    ValueError for anything the library would refuse.  Needs no device."""
    _ensemble.members(ensemble)
    return int(ensemble)


def tiling_argument(H: int, W: int, tile_h, tile_w, pad=0, batch=0) -> Tuple[int, int, int, int]:
    """The tiling of ``set_tiling`` for a session of H x W as ``(tile_h, tile_w, pad, batch)``; ValueError for anything the library would
    refuse (pfnl_amd/tiles.py ``check``).  Needs no device."""
    return _tiles.check(int(H), int(W), (tile_h, tile_w, pad, batch))


def frame_shapes(pixel_format: str, H: int, W: int, chroma: str = "420") -> Tuple[tuple, ...]:
    """The shapes a frame of H x W pixels may have: ``(H, W, 3)`` for rgb24 and rgb10; ``(H*3//2, W)`` or flat for the 4:2:0 formats
    (in samples: uint8, or uint16 for the 10-bit formats - ``frame_dtype``); ``(2*H, W)`` / ``(3*H, W)`` or flat with ``chroma`` "422" /
    "444"."""
    chroma_arguments(chroma)
    if pixel_format in ("rgb24", "rgb10"):
        return ((H, W, 3),)
    rows = {"420": H * 3 // 2, "422": 2 * H, "444": 3 * H}[chroma]
    return ((rows, W), (rows * W,))


def frame_dtype(pixel_format: str):
    """numpy's type of one sample: uint16 for rgb10 / p010 / i010, uint8 otherwise."""
    return np.uint16 if pixel_format in _capi.TEN_BIT_FORMATS else np.uint8


class VideoStream:
    """One open session on an engine (``PFNLEngine.open_stream`` / ``PFNL.open_stream``); an engine has one at a time.

    ``push(frame)`` takes a [H,W,3] uint8 numpy array or a uint8 torch tensor on the engine's device and returns the SR frames that
    have become deliverable as a list of ``(index, frame)`` - numpy in, numpy out; device tensor in, device tensors out.  Device
    tensors are read and written on the stream that was torch's current stream when the session was opened.

    ``scene_cut``: None - one scene, the reference's windows; ``"manual"`` - scenes begin where ``mark_cut()`` says; a float - a mean
    luma difference in (0, 255] for the detector (pfnl_amd/scene.py cut_rule), marks included.

    ``pixel_format`` / ``out_format`` ("rgb24" | "nv12" | "i420"; ``out_format`` None = the same): what ``push`` takes and ``pop`` returns.
    The 4:2:0 frames are tightly packed, ``(H*3//2, W)`` or flat in, ``(sH*3//2, sW)`` out (pfnl_amd/yuv.py), converted with ``matrix``
    ("bt601" | "bt709") at limited or ``full_range``.

    ``out_format`` "rgb10" | "p010" | "i010": ``pop`` returns uint16 frames (``torch.uint16`` on the device), 10-bit values by the rule of
    pfnl_amd/depth10.py - p010 in the upper ten bits of each sample; ``pixel_format`` takes none of them.

    ``in_depth`` (8 | 10): at 10, ``push`` and ``push_planes`` take uint16 frames (numpy, or ``torch.uint16`` on the device) in
    ``pixel_format``'s layout - "rgb24" values 0 .. 1023, "nv12" as P010, "i420" as I010 (pfnl_amd/depth10.py values10 / to_rgb10); ``cuts`` and
    ``last_info`` keep their meaning (pfnl_amd/scene.py luma_u10).

    ``out_size`` (None | ``(oH, oW)``): the raster ``pop`` delivers, ``(oH, oW, 3)`` or ``(oH*3//2, oW)``, by the rule of pfnl_amd/resize.py;
    each axis between a quarter and twice the network's output, even in a 4:2:0 output format.

    ``crop`` / ``fit`` / ``place`` / ``sar`` / ``fill`` (placement_arguments; pfnl_amd/fit.py): the rectangle ``crop`` of the SR raster
    resampled into a rectangle of the ``out_size`` canvas - the one ``fit`` ("contain" | "cover", with the sample aspect ratio ``sar``) works
    out, or ``place`` itself - and the 8-bit colour ``fill`` elsewhere.  ``crop`` alone delivers the crop at its own size.  With any of the
    three set, ``vs.crop`` and ``vs.place`` are the resolved rectangles and ``vs.out_size`` the canvas; else they are None.

    ``ensemble`` (1 | 2 | 4 | 8): every batch's forward as a geometric self-ensemble of that many members (pfnl_amd/ensemble.py); 1 is off.

    ``chroma_siting`` / ``out_chroma_siting`` ("left" | "center" | "topleft"; ``out_chroma_siting`` None = the same): where the chroma
    samples of a 4:2:0 ``pixel_format`` / ``out_format`` sit (pfnl_amd/yuv.py SITINGS); an RGB side ignores its siting.

    ``chroma`` / ``out_chroma`` ("420" | "422" | "444"; ``out_chroma`` None = the same): how the chroma planes of a YUV ``pixel_format`` /
    ``out_format`` are subsampled (pfnl_amd/yuv.py CHROMAS) - frames of ``(2*H, W)`` / ``(3*H, W)`` samples at "422" / "444"; an RGB side
    ignores it.  ``vs.chroma`` / ``vs.out_chroma`` are the resolved names.

    ``packing`` / ``out_packing`` (None | a name of pfnl_amd/packed.py PACKINGS; independent): ``push`` takes and ``pop`` returns one plane
    of interleaved samples - uint8 ``packed.frame_shape`` or flat - and ``push_planes`` / ``pop_planes`` the one plane ``(H, row bytes)`` with
    a pitch of its own.  A packing goes with the family, depth and chroma format of its side (packing_arguments).

    ``interlaced`` (None | "frame" | "field") with ``field_order`` ("tff" | "bff"): every pushed frame is woven - two fields in the pushed
    layout, whatever it is - and is deinterlaced on the device ahead of the ring (pfnl_amd/deinterlace.py): indices then count progressive
    frames, one per pushed frame at "frame" and two at "field".  A frame is made when the one after it has been pushed, or at ``end()``;
    4:2:0 planes need H to be a multiple of 4.  ``mark_cut()`` marks the next pushed frame and lands on the first frame made from it.

    ``telecine`` (None | "match" | "decimate") with ``field_order`` and ``telecine_params`` (None | a dict with "threshold", "post",
    "comb_limit"): every pushed frame is two fields of film under 3:2 pulldown; the fields are re-paired on the device ahead of the ring
    (pfnl_amd/telecine.py) and, at "decimate", one frame in five - the repeat - is dropped, so indices count film frames and a cycle's four
    frames come together; it needs a batch of at least 2.  Exclusive with ``interlaced``.  ``telecine_stats()`` counts the current sequence's frames.

    ``out_matrix`` / ``out_full_range`` / ``primaries`` / ``out_primaries`` (None = the input's; primaries "bt709" | "bt601-525" |
    "bt601-625"): the colour of each side (pfnl_amd/colour.py).  ``matrix`` and ``full_range`` then describe the input, the ``out_`` pair
    the delivered frames; where the primaries differ the SR frames are converted on the device in linear light, in the launch that
    quantises them, and everything behind - size, placement, ``fill``, YUV, packing - is in the output's colours.  ``vs.out_matrix``,
    ``vs.out_full_range``, ``vs.primaries`` and ``vs.out_primaries`` are the resolved values.

    ``bars`` (None | a limit in 0 .. 219; 8 is the usual one): every ring frame - behind the decode, the deinterlacer or inverse telecine -
    is measured on the device for letterbox and pillarbox bars (pfnl_amd/bars.py); ``vs.last_info["box"]`` is the box (y0, x0, h, w) of
    the frame the last pop delivered and ``vs.content_box`` the union over the frames popped so far in the sequence (None before the
    first).  The frames and the SR output are untouched: a crop ahead of the network is the caller's (python -m pfnl_amd.upscale --crop).

    ``set_tiling(tile_h, tile_w, pad=0, batch=0)``, before the first frame of a sequence: every batch's forward as runs of overlapping tiles
    (pfnl_amd/tiles.py); ``vs.tiling`` is the setting, None while off."""

    def __init__(self, engine, H: int, W: int, batch: int = 1, scene_cut=None, pixel_format="rgb24", out_format=None, matrix="bt709",
                 full_range=False, out_size=None, crop=None, fit=None, place=None, sar=(1, 1), fill=(0, 0, 0),
                 chroma_siting="left", out_chroma_siting=None, in_depth=8, chroma="420", out_chroma=None, packing=None,
                 out_packing=None, interlaced=None, field_order="tff", telecine=None, telecine_params=None, out_matrix=None,
                 out_full_range=None, primaries="bt709", out_primaries=None, bars=None, ensemble=1):
        import torch
        self.in_depth = depth_argument(in_depth)    # (before the engine is touched, as every check of an argument)
        self.bars = bars_argument(bars, H, W)
        col = colour_arguments(matrix, full_range, out_matrix, out_full_range, primaries, out_primaries)
        self.out_matrix = matrix if out_matrix is None else out_matrix
        self.out_full_range = bool(full_range if out_full_range is None else out_full_range)
        self.primaries, self.out_primaries = primaries, primaries if out_primaries is None else out_primaries
        il = interlace_arguments(interlaced, field_order, H, pixel_format, chroma, packing)
        tc = telecine_arguments(telecine, field_order, telecine_params, H, W, pixel_format, chroma, packing, interlaced)
        self.telecine = telecine
        self.interlaced, self.field_order = interlaced, field_order
        fmt = format_arguments(pixel_format, out_format, matrix, full_range)
        sub = chroma_arguments(chroma, out_chroma)
        self.chroma, self.out_chroma = chroma, chroma if out_chroma is None else out_chroma
        sit = siting_arguments(chroma_siting, out_chroma_siting)
        self.chroma_siting, self.out_chroma_siting = chroma_siting, chroma_siting if out_chroma_siting is None else out_chroma_siting
        self.ensemble = ensemble_argument(ensemble)
        self.pixel_format, self.out_format = pixel_format, pixel_format if out_format is None else out_format
        oH, oW, self.crop, self.place, self.fill = placement_arguments(out_size, engine.geom.scale * int(H), engine.geom.scale * int(W),
                                                                       self.out_format, crop, fit, place, sar, fill, self.out_chroma)
        self.out_size = (oH, oW) if oH else None
        pk = packing_arguments(packing, out_packing, pixel_format, self.out_format, self.in_depth, self.chroma, self.out_chroma, int(W),
                               oW if oH else engine.geom.scale * int(W))
        self.packing, self.out_packing = (None if packing == "none" else packing), (None if out_packing == "none" else out_packing)
        self.fit, self.sar = fit, tuple(sar)
        self.matrix, self.full_range = matrix, bool(full_range)
        if not engine._ready:
            raise RuntimeError("weights have not been loaded")
        self._engine = engine                       # (keeps the handle alive)
        self._lib = engine._lib
        self.H, self.W, self.batch = int(H), int(W), int(batch)
        self.scale = engine.geom.scale
        self.device = torch.device("cuda", engine.device)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        s = C.c_void_p()
        _capi.check(self._lib.pfnl_stream_open(engine._h, self.H, self.W, self.batch, C.c_void_p(stream) if stream else None, C.byref(s)))
        self._s = s
        self._device_frames = False                 # the container of the last pushed frame decides that of the popped ones
        self.scene_cut = scene_cut
        self.cuts: List[int] = []                   # delivered frames > 0 that start a scene
        self.last_info = None                       # (scene_first, sad) of the frame the last pop delivered
        if scene_cut is not None:
            try:
                if isinstance(scene_cut, str):
                    if scene_cut != "manual":
                        raise ValueError(f'scene_cut: None, "manual" or a threshold in (0, 255], got {scene_cut!r}')
                    _capi.check(self._lib.pfnl_stream_scenes(s, 1, 0.0))
                else:
                    _capi.check(self._lib.pfnl_stream_scenes(s, 2, float(scene_cut)))
            except Exception:
                self.close()
                raise
        if self.in_depth != 8:                      # (8: the session as it always was, and no call)
            try:
                _capi.check(self._lib.pfnl_stream_input_depth(s, self.in_depth))
            except Exception:
                self.close()
                raise
        if fmt[0] or fmt[1]:                        # (all defaults: the session as it always was, and no call)
            try:
                _capi.check(self._lib.pfnl_stream_format(s, *fmt))
            except Exception:
                self.close()
                raise
        if col is not None:                         # (one colour for both sides, BT.709 primaries: the session as it always was, and no
            try:                                    # call; behind the format, which sets matrix and range of both sides)
                _capi.check(self._lib.pfnl_stream_colour(s, C.byref(_capi.pfnl_colour(*col[0])), C.byref(_capi.pfnl_colour(*col[1]))))
            except Exception:
                self.close()
                raise
        if sit[0] or sit[1]:                        # (left on both sides: the session as it always was, and no call)
            try:
                _capi.check(self._lib.pfnl_stream_chroma_siting(s, *sit))
            except Exception:
                self.close()
                raise
        if sub[0] or sub[1]:                        # (4:2:0 on both sides: the session as it always was, and no call)
            try:
                _capi.check(self._lib.pfnl_stream_chroma_format(s, *sub))
            except Exception:
                self.close()
                raise
        if self.out_size is not None:               # (behind the format: the size is checked against it)
            try:
                if self.place is None:
                    _capi.check(self._lib.pfnl_stream_resize(s, *self.out_size))
                else:
                    _capi.check(self._lib.pfnl_stream_place(s, *self.out_size, _capi.rect_arg(self.crop), _capi.rect_arg(self.place),
                                                            (C.c_uint8 * 3)(*self.fill)))
            except Exception:
                self.close()
                raise
        if pk[0] or pk[1]:                          # (planes on both sides: the session as it always was, and no call; behind every setting
            try:                                    # a packing is checked against)
                _capi.check(self._lib.pfnl_stream_packing(s, *pk))
            except Exception:
                self.close()
                raise
        if self.ensemble != 1:                      # (1: the session as it always was, and no call)
            try:
                _capi.check(self._lib.pfnl_stream_ensemble(s, self.ensemble))
            except Exception:
                self.close()
                raise
        if il[0]:                                   # (None: the session as it always was, and no call; behind the input setting it is checked
            try:                                    # against, and the depth its field store follows)
                _capi.check(self._lib.pfnl_stream_interlace(s, *il))
            except Exception:
                self.close()
                raise
        if tc[0]:                                   # (None: the session as it always was, and no call; behind the input setting, as above)
            try:
                _capi.check(self._lib.pfnl_stream_telecine(s, tc[0], tc[1], C.byref(_capi.pfnl_telecine_params(*tc[2]))))
            except Exception:
                self.close()
                raise
        if self.bars is not None:                   # (None: the session as it always was, and no call)
            try:
                _capi.check(self._lib.pfnl_stream_bars(s, 1, self.bars))
            except Exception:
                self.close()
                raise

    # ---- lifetime --------------------------------------------------------------------------
    def close(self) -> None:
        """Drops what was not popped, restores the options a range recovery changed, frees the session's buffers."""
        if getattr(self, "_s", None):
            s, self._s = self._s, None
            if getattr(self._engine, "_h", None):   # (a closed engine has closed its session with it)
                _capi.check(self._lib.pfnl_stream_close(s))

    def __enter__(self) -> "VideoStream":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if not getattr(self, "_s", None):
            raise RuntimeError("the stream is closed")
        if not getattr(self._engine, "_h", None):   # the engine destroyed its handle, and the session with it
            self._s = None
            raise RuntimeError("the stream's engine has been closed")
        return self._s

    # ---- frames ----------------------------------------------------------------------------
    def push(self, frame) -> List[tuple]:
        """Hands one LR frame over and returns the SR frames of the batches launched BEFORE this push (possibly none).  A batch this
        push launches is left running - its frames come with the next push or with ``end()`` - so the GPU works on it while the caller
        fetches the next frame (``pop`` is there for a caller that wants them at once)."""
        s = self._handle()
        due = self.ready()
        if self.packing is not None:
            frame = packed_frame_argument(frame, self.packing, self.H, self.W)
        else:
            frame = frame_argument(frame, self.pixel_format, self.H, self.W, self.in_depth, self.chroma)
        if type(frame).__module__.startswith("torch"):
            if not frame.is_cuda or frame.device.index != self.device.index:
                raise ValueError(f"tensor on {frame.device}, stream on {self.device} (host frames: numpy arrays)")
            self._device_frames = True
            return self._hand_over(lambda: self._lib.pfnl_stream_push(s, C.c_void_p(frame.data_ptr()), 1), due)
        self._device_frames = False
        return self._hand_over(lambda: self._lib.pfnl_stream_push(s, frame.ctypes.data_as(C.c_void_p), 0), due)

    def _hand_over(self, call, due, container=None) -> List[tuple]:
        """``call`` pushes the frame; then the ``due`` frames are popped.  An interlaced session admits up to two ring frames per push, so
        the library may ask for the due frames first ("pop first": it has changed nothing): they are popped, the push is repeated, and
        they are returned from this call all the same.  A progressive session's calls are what they always were.  ``container``: what
        ``_device_frames`` becomes once the frame has been taken (None: the caller has set it)."""
        try:
            _capi.check(call())
        except _capi.PFNLHipError as e:
            if (self.interlaced is None and self.telecine is None) or "pop first" not in str(e):
                raise
            if container is not None:
                self._device_frames = container
            frames = self.pop_ready(due)
            _capi.check(call())
            return frames
        if container is not None:
            self._device_frames = container
        return self.pop_ready(due)

    def end(self) -> List[tuple]:
        """No more frames: the remaining windows clamp at the last one.  Returns the remaining SR frames."""
        s = self._handle()
        try:
            _capi.check(self._lib.pfnl_stream_end(s))
        except _capi.PFNLHipError as e:             # (an interlaced session's held frame did not fit: what is ready is popped, once)
            if (self.interlaced is None and self.telecine is None) or "pop first" not in str(e):
                raise
            frames = self.pop_ready()
            _capi.check(self._lib.pfnl_stream_end(s))
            return frames + self.pop_ready()
        return self.pop_ready()

    def reset(self) -> None:
        """The next sequence, same geometry, scene setting, formats and output size; what was not popped is dropped, and so are a pending
        mark and ``cuts``."""
        _capi.check(self._lib.pfnl_stream_reset(self._handle()))
        self.cuts = []
        self.last_info = None

    @property
    def content_box(self):
        """With ``bars``: the union (y0, x0, h, w) of the content boxes of the frames popped so far in the sequence - (0, 0, 0, 0) while
        all were black -, or None before the first pop and without ``bars``."""
        if self.bars is None or self.last_info is None:
            return None
        box, n = (C.c_int32 * 4)(), C.c_longlong(0)
        _capi.check(self._lib.pfnl_stream_content_box(self._handle(), box, C.byref(n)))
        return tuple(int(v) for v in box)

    @property
    def tiling(self):
        """``(tile_h, tile_w, pad, batch)`` as ``set_tiling`` stored it, or None: whole frames."""
        return getattr(self, "_tiling", None)

    def set_tiling(self, tile_h, tile_w, pad=0, batch=0) -> None:
        """Every batch's forward as runs of ``batch`` overlapping tiles of tile_h x tile_w with margin ``pad`` (pfnl_stream_tile; the rule:
        pfnl_amd/tiles.py; batch 0: all tiles of a batch of windows in one run).  ``set_tiling(None, None)`` turns it off.  Accepted only
        before the first frame of a sequence; the setting survives ``reset``."""
        if tile_h is None and tile_w is None:
            _capi.check(self._lib.pfnl_stream_tile(self._handle(), None))
            self._tiling = None
            return
        t = tiling_argument(self.H, self.W, tile_h, tile_w, pad, batch)          # (before anything touches the session)
        _capi.check(self._lib.pfnl_stream_tile(self._handle(), C.byref(_capi.pfnl_tiling(*t))))
        self._tiling = t

    def telecine_stats(self) -> dict:
        """The current sequence's frames so far: matched as pushed ("c"), matched with the field before ("p"), post-processed as video,
        dropped, and admitted to the ring (pfnl_stream_telecine_stats; all 0 without ``telecine``)."""
        out = (C.c_longlong * 5)()
        _capi.check(self._lib.pfnl_stream_telecine_stats(self._handle(), out))
        return dict(zip(("matched_c", "matched_p", "post", "dropped", "delivered"), (int(v) for v in out)))

    def mark_cut(self) -> None:
        """The next pushed frame starts a scene (needs ``scene_cut``; before the first frame of a sequence it changes nothing)."""
        _capi.check(self._lib.pfnl_stream_mark_cut(self._handle()))

    def ready(self) -> int:
        """SR frames that ``pop`` would deliver without another push."""
        n = C.c_int(0)
        _capi.check(self._lib.pfnl_stream_ready(self._handle(), C.byref(n)))
        return n.value

    def pop(self):
        """The next SR frame as ``(index, frame)``, or None when none is deliverable; waits only for the batch that holds it."""
        s = self._handle()
        oH, oW = self.out_size if self.out_size is not None else (self.scale * self.H, self.scale * self.W)
        shape = frame_shapes(self.out_format, oH, oW, self.out_chroma)[0]
        index, got = C.c_longlong(0), C.c_int(0)
        ten = self.out_format in _capi.TEN_BIT_FORMATS
        if self.out_packing is not None:            # (bytes, whatever the unit)
            from . import packed as _packed
            shape, ten = _packed.frame_shape(self.out_packing, oH, oW), False
        if self._device_frames:
            import torch
            out = torch.empty(shape, dtype=torch.uint16 if ten else torch.uint8, device=self.device)
            _capi.check(self._lib.pfnl_stream_pop(s, C.c_void_p(out.data_ptr()), 1, C.byref(index), C.byref(got)))
        else:
            out = np.empty(shape, np.uint8 if self.out_packing is not None else frame_dtype(self.out_format))
            _capi.check(self._lib.pfnl_stream_pop(s, out.ctypes.data_as(C.c_void_p), 0, C.byref(index), C.byref(got)))
        if not got.value:
            return None
        self._note_info(s, index.value)
        return index.value, out

    def _note_info(self, s, index: int) -> None:
        """``last_info`` and ``cuts`` for the frame a pop has just delivered."""
        if self.scene_cut is not None:
            first, sad = C.c_longlong(0), C.c_ulonglong(0)
            _capi.check(self._lib.pfnl_stream_pop_info(s, C.byref(first), C.byref(sad)))
            self.last_info = (first.value, sad.value)
            if index > 0 and first.value == index:
                self.cuts.append(index)
        else:
            self.last_info = (0, 0)
        if self.bars is not None:
            box = (C.c_int32 * 4)()
            _capi.check(self._lib.pfnl_stream_pop_box(s, box))
            self.last_info = PopInfo(*self.last_info, (int(v) for v in box))

    # ---- surfaces: planes with a row pitch (pfnl_amd/surface.py) -------------------------------
    def _planes_struct(self, planes, fmt, H, W, chroma="420", packing=None):
        """(pfnl_surface, on the device?) of a tuple of planes, all numpy arrays or all tensors on the stream's device."""
        on_device = [type(p).__module__.startswith("torch") for p in planes]
        if any(on_device) != all(on_device):
            raise ValueError("the planes of a frame are all numpy arrays or all device tensors")
        if planes and on_device[0]:
            for p in planes:
                if not p.is_cuda or p.device.index != self.device.index:
                    raise ValueError(f"tensor on {p.device}, stream on {self.device} (host planes: numpy arrays)")
        return _surface.as_struct(planes, fmt, H, W, chroma, packing), bool(planes) and on_device[0]

    def push_planes(self, *planes) -> List[tuple]:
        """``push`` of a frame given as its planes in ``pixel_format`` - (Y, CbCr) for nv12, (Y, Cb, Cr) for i420, one (H, W, 3) or (H, 3 W)
        plane for rgb24; uint16 samples at an input depth of 10 - each a numpy array or each a device tensor, with whatever row pitch its strides say (pfnl_amd/surface.py):
        typically views ``surface[:H, :W]`` of a decoder's pitched surface, which is read where it lies.  Returns what ``push`` returns;
        the two may alternate within a sequence."""
        s = self._handle()
        sf, on_device = self._planes_struct(planes, pushed_format(self.pixel_format, self.in_depth), self.H, self.W, self.chroma,
                                            self.packing)
        due = self.ready()
        return self._hand_over(lambda: self._lib.pfnl_stream_push_surface(s, C.byref(sf), 1 if on_device else 0), due, on_device)

    def pop_planes(self, *planes):
        """``pop`` into planes the caller owns, in ``out_format`` at the output size - numpy arrays or device tensors with a row pitch of
        their own, an encoder's surface: only the samples are written, never the bytes between a row's end and the pitch.  Returns the
        frame's index, or None when no frame is deliverable (then nothing was written)."""
        s = self._handle()
        oH, oW = self.out_size if self.out_size is not None else (self.scale * self.H, self.scale * self.W)
        sf, on_device = self._planes_struct(planes, self.out_format, oH, oW, self.out_chroma, self.out_packing)
        for p in planes:
            if not on_device and not p.flags.writeable:
                raise ValueError("pop_planes writes into its planes: a read-only array")
        index, got = C.c_longlong(0), C.c_int(0)
        _capi.check(self._lib.pfnl_stream_pop_surface(s, C.byref(sf), 1 if on_device else 0, C.byref(index), C.byref(got)))
        if not got.value:
            return None
        self._note_info(s, index.value)
        return index.value

    def pop_ready(self, limit=None) -> List[tuple]:
        frames = []
        for _ in range(self.ready() if limit is None else limit):
            item = self.pop()
            if item is None:
                break
            frames.append(item)
        return frames
