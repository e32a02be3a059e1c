"""Surfaces: a frame as one array per plane, each with a row pitch of its own (include/pfnl_hip.h SURFACES; the C side of this rule is
pfnl_amd/csrc/surface_geom.h).  numpy only, no device.

A hardware decoder or encoder hands out no packed frame.  Its surface is a pointer per plane and a pitch per plane - rounded up to 64 or 256
bytes, under a coded height above the displayed one - and the natural Python picture of that is a strided view, ``surface[:H, :W]`` of the
pitched allocation.  ``describe`` turns a tuple of such views (numpy arrays, or anything with ``data_ptr`` / ``stride`` / ``element_size``:
a torch tensor) into the pointers and pitches of a ``pfnl_surface``; ``embed`` / ``views`` / ``extract`` build pitched buffers and read
them back, which is what the tests do with them.

Planes of a frame of H x W (``plane_shapes``): rgb24 / rgb10 one plane of H rows of 3 W samples; nv12 / p010 Y with H rows of W and CbCr
with H/2 rows of W (W/2 interleaved pairs); i420 / i010 Y, then Cb and Cr with H/2 rows of W/2 each.  uint8 samples, uint16 for the 10-bit
formats.  With ``chroma`` "422" / "444" (pfnl_amd/yuv.py CHROMAS) the chroma planes of a YUV format have H rows - of W / 2 samples (CbCr: W)
at 4:2:2, of W (CbCr: 2 W) at 4:4:4 - and W alone is even at 4:2:2, nothing at 4:4:4; an RGB format ignores it.  A plane may be given with its row split into further axes - ``(H, W, 3)``, ``(H/2, W/2, 2)`` - as long as a row is contiguous.

With ``packing`` (pfnl_amd/packed.py PACKINGS) the frame is ONE plane of H rows of ``packed.row_bytes`` bytes, uint8 whatever the unit, and
``fmt`` says no more than the side's family and depth, which must agree with the packing.

A window of a larger surface is just a view that starts at the window's first sample (even x and y): the frame is then that window."""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence, Tuple

import numpy as np

from . import _capi


def plane_shapes(fmt: str, H: int, W: int, chroma: str = "420", packing=None) -> Tuple[tuple, ...]:
    """Per plane of a frame of H x W in ``fmt``: (rows, samples per row, numpy dtype of a sample).  ``packing``: the one plane of a packed
    format, in bytes."""
    from . import yuv as _yuv
    if fmt not in _capi.PIXEL_FORMATS:
        raise ValueError(f"fmt: one of {sorted(_capi.PIXEL_FORMATS)}, got {fmt!r}")
    H, W = int(H), int(W)
    if packing not in (None, "none"):
        from . import packed as _packed
        _packed.check(packing, H, W)
        why = _packed.side_refused(packing, fmt in _capi.FORMATS_420, 10 if fmt in _capi.TEN_BIT_FORMATS else 8, chroma, W)
        if why:
            raise ValueError(why)
        return ((H, _packed.row_bytes(packing, W), np.dtype(np.uint8)),)
    is_yuv = fmt in _capi.FORMATS_420                   # (the YUV layouts: 4:2:0 unless ``chroma`` says otherwise)
    if H < 1 or W < 1 or (is_yuv and chroma == "420" and (H % 2 or W % 2)):
        raise ValueError(f"H and W must be positive, and even for a 4:2:0 format, got {H} x {W}")
    dt = np.dtype(np.uint16 if fmt in _capi.TEN_BIT_FORMATS else np.uint8)
    if fmt in ("rgb24", "rgb10"):
        _yuv.chroma_id(chroma)
        return ((H, 3 * W, dt),)
    _yuv.check_size(H, W, chroma)
    ch, cw = _yuv.chroma_shape(H, W, chroma)
    if fmt in ("nv12", "p010"):
        return ((H, W, dt), (ch, 2 * cw, dt))
    return ((H, W, dt), (ch, cw, dt), (ch, cw, dt))


def _layout(a):
    """(address, shape, strides in bytes, item size, dtype name) of a numpy array or a tensor-like object."""
    if hasattr(a, "data_ptr") and hasattr(a, "stride") and hasattr(a, "element_size"):
        es = int(a.element_size())
        return int(a.data_ptr()), tuple(int(n) for n in a.shape), tuple(int(v) * es for v in a.stride()), es, str(a.dtype).replace("torch.", "")
    if not isinstance(a, np.ndarray):
        raise ValueError(f"a plane is a numpy array or a tensor with data_ptr / stride / element_size, got {type(a).__name__}")
    return int(a.ctypes.data), a.shape, a.strides, a.dtype.itemsize, a.dtype.name


def describe(arrays: Sequence, fmt: str, H: int, W: int, chroma: str = "420", packing=None) -> Tuple[List[int], List[int]]:
    """(pointers, pitches in bytes) of the planes ``arrays`` hold for a frame of H x W in ``fmt``.  ValueError for a wrong plane count, a
    wrong dtype or shape, a row that is not contiguous (last-axis stride other than one sample), a negative stride, a row stride below
    the bytes of a row."""
    shapes = plane_shapes(fmt, H, W, chroma, packing)
    arrays = tuple(arrays)
    if len(arrays) != len(shapes):
        raise ValueError(f"{fmt} has {len(shapes)} plane(s), got {len(arrays)}")
    pointers, pitches = [], []
    for k, (a, (rows, samples, dt)) in enumerate(zip(arrays, shapes)):
        ptr, shape, strides, es, name = _layout(a)
        if name != dt.name:
            raise ValueError(f"plane {k}: expected {dt.name} samples, got {name}")
        if len(shape) < 2 or shape[0] != rows or int(np.prod(shape[1:], dtype=np.int64)) != samples:
            raise ValueError(f"plane {k}: expected {rows} rows of {samples} samples, got shape {tuple(shape)}")
        if any(v < 0 for v in strides):
            raise ValueError(f"plane {k}: negative stride {tuple(strides)}")
        want = es                                      # a row is contiguous: from the last axis up, each stride is the extent below it
        for n, v in zip(shape[:0:-1], strides[:0:-1]):
            if v != want and n != 1:
                raise ValueError(f"plane {k}: a row must be contiguous (last-axis stride of one sample), got strides {tuple(strides)} bytes")
            want *= n
        pitch = strides[0] if rows > 1 else max(strides[0], samples * es)
        if pitch < samples * es:
            raise ValueError(f"plane {k}: row pitch {pitch} is below the {samples * es} bytes of a row")
        pointers.append(ptr)
        pitches.append(pitch)
    return pointers, pitches


def as_struct(arrays: Sequence, fmt: str, H: int, W: int, chroma: str = "420", packing=None) -> "_capi.pfnl_surface":
    """``describe`` as the ``pfnl_surface`` the library takes (the arrays must outlive the call it is passed to)."""
    pointers, pitches = describe(arrays, fmt, H, W, chroma, packing)
    pad = 3 - len(pointers)
    return _capi.pfnl_surface((C.c_void_p * 3)(*pointers, *([None] * pad)), (C.c_size_t * 3)(*pitches, *([0] * pad)))


def split(frame, fmt: str, H: int, W: int, chroma: str = "420") -> List[np.ndarray]:
    """The planes of one tightly packed frame (what ``push`` takes and ``pop`` returns; any shape with the frame's samples) as
    (rows, samples) views: the packed frame is its planes one behind the other."""
    shapes = plane_shapes(fmt, H, W, chroma)
    flat = np.asarray(frame).reshape(-1)
    if flat.dtype != shapes[0][2] or flat.size != sum(rows * n for rows, n, _ in shapes):
        raise ValueError(f"expected {sum(rows * n for rows, n, _ in shapes)} {shapes[0][2].name} samples, got {flat.size} {flat.dtype.name}")
    out, at = [], 0
    for rows, n, _ in shapes:
        out.append(flat[at:at + rows * n].reshape(rows, n))
        at += rows * n
    return out


def embed(planes: Sequence[np.ndarray], pitches: Sequence[int], fill: int = 0) -> List[np.ndarray]:
    """One pitched buffer per plane: uint8 ``[rows, pitch]`` holding ``fill`` with the plane's rows at the row starts.  ``planes`` are
    2-D (rows, samples) arrays; a pitch below the bytes of a row is a ValueError."""
    planes, pitches = list(planes), [int(p) for p in pitches]
    if len(planes) != len(pitches):
        raise ValueError(f"{len(planes)} plane(s) and {len(pitches)} pitch(es)")
    out = []
    for k, (p, pitch) in enumerate(zip(planes, pitches)):
        p = np.ascontiguousarray(p)
        if p.ndim != 2:
            raise ValueError(f"plane {k}: expected (rows, samples), got shape {p.shape}")
        row = p.shape[1] * p.dtype.itemsize
        if pitch < row or pitch % p.dtype.itemsize:
            raise ValueError(f"plane {k}: pitch {pitch} for rows of {row} bytes of {p.dtype.name}")
        buf = np.full((p.shape[0], pitch), fill, np.uint8)
        buf[:, :row] = p.view(np.uint8).reshape(p.shape[0], row)
        out.append(buf)
    return out


def views(buffers: Sequence, fmt: str, H: int, W: int, chroma: str = "420", packing=None) -> list:
    """The planes inside pitched buffers (uint8 ``[rows, pitch]``, numpy or tensors): strided (rows, samples) views in the format's sample
    type, sharing the buffers' memory - what ``describe``, ``VideoStream.push_planes`` and ``pop_planes`` take."""
    shapes = plane_shapes(fmt, H, W, chroma, packing)
    buffers = list(buffers)
    if len(buffers) != len(shapes):
        raise ValueError(f"{fmt} has {len(shapes)} plane(s), got {len(buffers)} buffer(s)")
    out = []
    for k, (b, (rows, samples, dt)) in enumerate(zip(buffers, shapes)):
        row = samples * dt.itemsize
        if len(b.shape) != 2 or b.shape[0] < rows or b.shape[1] < row:
            raise ValueError(f"buffer {k}: expected at least {rows} rows of {row} bytes, got shape {tuple(b.shape)}")
        v = b[:rows, :row]
        if dt.itemsize > 1:
            v = v.view(dt) if isinstance(v, np.ndarray) else v.view(getattr(__import__("torch"), dt.name))
        out.append(v)
    return out


def extract(buffers: Sequence[np.ndarray], fmt: str, H: int, W: int, chroma: str = "420") -> List[np.ndarray]:
    """The planes of pitched numpy buffers as contiguous (rows, samples) arrays of their own."""
    return [np.ascontiguousarray(v) for v in views(buffers, fmt, H, W, chroma)]
