"""Packed formats: one plane whose samples are interleaved within a pixel or a pixel group (numpy only; no device).

What a capture card (yuyv422 = YUY2, uyvy422), an SDI card or a QuickTime / MXF master (v210), and a swap chain (bgra / rgba, x2rgb10 /
x2bgr10, y210) hand over.  The streaming session takes and delivers them (include/pfnl_hip.h PACKED FORMATS, pfnl_stream_packing;
pfnl_amd/csrc/packed.hip, the C side of the table: pfnl_amd/csrc/pack_geom.h), and this module is the rule its kernels are tested against,
byte for byte.  There is NO new arithmetic here: a packing is a LAYOUT, and the rule is ``unpack``, then the existing one - pfnl_amd/yuv.py
at 8 bits, pfnl_amd/depth10.py at 10, with ``chroma="422"`` - or that rule, then ``pack``.

The table (``PACKINGS``; the index is the C-ABI's PFNL_PACK_* value, 0 = "none" = the planes of the layout):

=========  ======================  ==========================================================  ==============
name       side must be            unit                                                        bytes of a row
=========  ======================  ==========================================================  ==============
bgr24      RGB, 8 bits             3 bytes B, G, R                                             3 W
rgba       RGB, 8 bits             4 bytes R, G, B, A                                          4 W
bgra       RGB, 8 bits             4 bytes B, G, R, A                                          4 W
yuyv422    YUV, 8 bits, 4:2:2      4 bytes Y0 Cb Y1 Cr per pixel pair                          2 W
uyvy422    YUV, 8 bits, 4:2:2      4 bytes Cb Y0 Cr Y1                                         2 W
x2rgb10    RGB, 10 bits            one little-endian uint32: bits 29..20 R, 19..10 G, 9..0 B   4 W
x2bgr10    RGB, 10 bits            uint32: bits 29..20 B, 19..10 G, 9..0 R                     4 W
y210       YUV, 10 bits, 4:2:2     four uint16 Y0 Cb Y1 Cr, the value in the upper ten bits    4 W
v210       YUV, 10 bits, 4:2:2,    16 bytes per 6 pixels: four little-endian uint32, each of   16 W / 6
           W a multiple of 6       three 10-bit samples at bits 9..0, 19..10, 29..20 -
                                   Cb0 Y0 Cr0 | Y1 Cb1 Y2 | Cr1 Y3 Cb2 | Y4 Cr2 Y5
=========  ======================  ==========================================================  ==============

A frame is ALWAYS a uint8 array ``(H, tight_row_bytes)`` - bytes, whatever the unit, so one shape serves every packing and a file or a
pipe; ``tight_row_bytes`` is the row bytes except for v210, whose rows are ((W + 47) // 48) * 128 bytes, the format's own rule.

Conventions: alpha and the two spare bits of an X2 word are ignored by ``unpack`` and written opaque by ``pack`` (255; 3); bits 31..30 of a
v210 word and the padding of a v210 row are written 0 and ignored; y210's low six bits are written 0 and ignored.  Sample values pass as
they come, 0 .. 1023 at 10 bits, no clamp to a legal range.  A 4:2:2 packing reads the horizontal half of a siting, as planar 4:2:2 does.

Out of scope: big-endian variants, 12 and 16 bits, packed 4:4:4, alpha carried through, v210 widths that are no multiple of 6.
"""
from __future__ import annotations

from typing import Tuple

import numpy as np

from . import depth10 as _d10
from . import yuv as _yuv

PACKINGS = ("none", "bgr24", "rgba", "bgra", "yuyv422", "uyvy422", "x2rgb10", "x2bgr10", "y210", "v210")   # PFNL_PACK_*: the index is the value
# name -> (family is YUV, bits, pixels of a unit, bytes of a unit, alignment of pointer and pitch)
TABLE = {
    "bgr24": (False, 8, 1, 3, 1), "rgba": (False, 8, 1, 4, 1), "bgra": (False, 8, 1, 4, 1),
    "yuyv422": (True, 8, 2, 4, 1), "uyvy422": (True, 8, 2, 4, 1),
    "x2rgb10": (False, 10, 1, 4, 4), "x2bgr10": (False, 10, 1, 4, 4),
    "y210": (True, 10, 2, 8, 2), "v210": (True, 10, 6, 16, 4),
}
_RGBA_ORDER = {"bgr24": (2, 1, 0), "rgba": (0, 1, 2), "bgra": (2, 1, 0)}     # the byte of R, G, B in a pixel
_X2_SHIFT = {"x2rgb10": (20, 10, 0), "x2bgr10": (0, 10, 20)}                 # the bit of R, G, B in a word
_YUYV_Y0 = {"yuyv422": 0, "uyvy422": 1}                                      # the byte of Y0 in a pair
# v210: (word, field) of Y0 .. Y5, Cb0 .. Cb2, Cr0 .. Cr2 in a group; a field is 10 bits at 10 * field
_V210_Y = ((0, 1), (1, 0), (1, 2), (2, 1), (3, 0), (3, 2))
_V210_CB = ((0, 0), (1, 1), (2, 2))
_V210_CR = ((0, 2), (2, 0), (3, 1))


def packing_id(name) -> int:
    """The C-ABI's PFNL_PACK_* value of a packing's name (None and "none": 0); ValueError for anything else."""
    if name is None:
        return 0
    if name not in PACKINGS:
        raise ValueError(f"packing: one of {PACKINGS}, got {name!r}")
    return PACKINGS.index(name)


def _entry(name):
    if packing_id(name) == 0:
        raise ValueError(f"packing: one of {PACKINGS[1:]}, got {name!r}")
    return TABLE[name]


def is_yuv(name) -> bool:
    return _entry(name)[0]


def bits(name) -> int:
    return _entry(name)[1]


def side_refused(name, family_is_yuv: bool, depth: int, chroma: str, W: int):
    """None where a side of this family, depth (8 | 10) and chroma format ("420" | "422" | "444") may carry the packing at a width of W;
    else the words that name what disagrees (pack_geom.h pack_refused, word for word).  "none" agrees with every side."""
    if packing_id(name) == 0:
        return None
    yuv, depth_of, unit_px, _, _ = TABLE[name]
    if yuv != bool(family_is_yuv):
        return ("packing: a YUV packing (yuyv422, uyvy422, y210, v210) needs a YUV family on its side, not RGB" if yuv else
                "packing: an RGB packing (bgr24, rgba, bgra, x2rgb10, x2bgr10) needs an RGB family on its side, not YUV")
    if depth_of != depth:
        return ("packing: an 8-bit packing (bgr24, rgba, bgra, yuyv422, uyvy422) needs a depth of 8 bits on its side" if depth_of == 8 else
                "packing: a 10-bit packing (x2rgb10, x2bgr10, y210, v210) needs a depth of 10 bits on its side")
    if yuv and chroma != "422":
        return "packing: a YUV packing needs the chroma format PFNL_CHROMA_422 on its side"
    if W < 1:
        return "packing: the width must be at least 1"
    if name == "v210" and W % 6:
        return "packing: v210 needs a width that is a multiple of 6"
    if yuv and W % 2:
        return "packing: a 4:2:2 packing needs an even width"
    return None


def check(name, H: int, W: int) -> None:
    """ValueError unless a frame of H x W exists in this packing: H, W >= 1, W even for a 4:2:2 packing, a multiple of 6 for v210."""
    yuv, depth, _, _, _ = _entry(name)
    why = side_refused(name, yuv, depth, "422", int(W))
    if why is None and H < 1:
        why = "packing: the height must be at least 1"
    if why:
        raise ValueError(f"{why} (got {H} x {W})")


def row_bytes(name, W: int) -> int:
    """The bytes of a row that hold samples."""
    check(name, 1, W)
    _, _, unit_px, unit_bytes, _ = TABLE[name]
    return W // unit_px * unit_bytes


def tight_row_bytes(name, W: int) -> int:
    """The row of a tightly packed frame: v210 rounds the width up to 48 pixels (128 bytes) - the format's own rule, which holds for any
    W >= 1 (1280 -> 3456), also where this module takes no frame of that width -; every other packing's is ``row_bytes``."""
    if name == "v210" and W >= 1:
        return (W + 47) // 48 * 128
    return row_bytes(name, W)


def frame_bytes(name, H: int, W: int) -> int:
    check(name, H, W)
    return H * tight_row_bytes(name, W)


def frame_shape(name, H: int, W: int) -> Tuple[int, int]:
    check(name, H, W)
    return (H, tight_row_bytes(name, W))


def frame_dtype(name):
    """uint8 for every packing: a frame is its bytes."""
    _entry(name)
    return np.dtype(np.uint8)


def _as_frame(frame, name, H, W):
    flat = np.asarray(frame).reshape(-1)
    if flat.dtype != np.uint8:
        flat = np.ascontiguousarray(flat).view(np.uint8)
    if flat.size != frame_bytes(name, H, W):
        raise ValueError(f"{name}: expected {frame_bytes(name, H, W)} bytes for {H} x {W}, got {flat.size}")
    return flat.reshape(frame_shape(name, H, W))[:, :row_bytes(name, W)]


def _words(rows, dtype):
    return np.ascontiguousarray(rows).view(dtype)


def unpack(frame, name, H: int, W: int):
    """A packed frame (``frame_shape`` bytes, any shape or a flat buffer) -> the sample VALUES.  RGB packings: ``(H, W, 3)`` R, G, B;
    YUV packings: ``(Y [H, W], Cb [H, W/2], Cr [H, W/2])``.  uint8 at 8 bits, uint16 in 0 .. 1023 at 10."""
    rows = _as_frame(frame, name, H, W)
    if name in _RGBA_ORDER:
        px = rows.reshape(H, W, -1)
        return np.stack([px[..., k] for k in _RGBA_ORDER[name]], axis=-1)
    if name in _X2_SHIFT:
        w = _words(rows, "<u4")
        return np.stack([(w >> sh) & 1023 for sh in _X2_SHIFT[name]], axis=-1).astype(np.uint16)
    if name in _YUYV_Y0:
        q, y0 = rows.reshape(H, W // 2, 4), _YUYV_Y0[name]
        return np.stack([q[..., y0], q[..., y0 + 2]], axis=-1).reshape(H, W), q[..., 1 - y0].copy(), q[..., 3 - y0].copy()
    if name == "y210":
        q = (_words(rows, "<u2") >> 6).reshape(H, W // 2, 4)
        return np.stack([q[..., 0], q[..., 2]], axis=-1).reshape(H, W), q[..., 1].copy(), q[..., 3].copy()
    g = _words(rows, "<u4").reshape(H, W // 6, 4)                       # v210
    take = lambda at: np.stack([(g[..., j] >> (10 * k)) & 1023 for j, k in at], axis=-1).reshape(H, -1).astype(np.uint16)   # noqa: E731
    return take(_V210_Y), take(_V210_CB), take(_V210_CR)


def _check_values(a, name, shape):
    a = np.asarray(a)
    top = (1 << bits(name)) - 1
    if a.shape != shape or a.dtype.kind not in "ui":
        raise ValueError(f"{name}: expected integer values of shape {shape}, got {a.dtype} {a.shape}")
    if a.size and (int(a.min()) < 0 or int(a.max()) > top):
        raise ValueError(f"{name}: values must lie in 0 .. {top}")
    return a.astype(np.uint32)


def pack(samples, name, H: int, W: int):
    """The inverse of ``unpack``: values -> the tightly packed frame, uint8 ``frame_shape``.  Alpha and spare bits opaque, v210's zero."""
    check(name, H, W)
    out = np.zeros(frame_shape(name, H, W), np.uint8)
    nb = row_bytes(name, W)
    if not is_yuv(name):
        rgb = _check_values(samples, name, (H, W, 3))
        if name in _RGBA_ORDER:
            px = np.full((H, W, TABLE[name][3]), 255, np.uint8)
            for ch, k in enumerate(_RGBA_ORDER[name]):
                px[..., k] = rgb[..., ch]
            out[:, :nb] = px.reshape(H, nb)
        else:
            sr, sg, sb = _X2_SHIFT[name]
            w = (rgb[..., 0] << sr) | (rgb[..., 1] << sg) | (rgb[..., 2] << sb) | np.uint32(0xC0000000)
            out[:, :nb] = w.astype("<u4").view(np.uint8).reshape(H, nb)
        return out
    Y, Cb, Cr = samples
    Y, Cb, Cr = _check_values(Y, name, (H, W)), _check_values(Cb, name, (H, W // 2)), _check_values(Cr, name, (H, W // 2))
    if name in _YUYV_Y0 or name == "y210":
        y0 = _YUYV_Y0.get(name, 0)
        q = np.zeros((H, W // 2, 4), np.uint32)
        q[..., y0], q[..., y0 + 2], q[..., 1 - y0], q[..., 3 - y0] = Y[:, 0::2], Y[:, 1::2], Cb, Cr
        q = q.astype(np.uint8) if name != "y210" else (q << 6).astype("<u2").view(np.uint8)
        out[:, :nb] = q.reshape(H, nb)
        return out
    g = np.zeros((H, W // 6, 4), np.uint32)                             # v210
    for plane, at in ((Y, _V210_Y), (Cb, _V210_CB), (Cr, _V210_CR)):
        p = plane.reshape(H, W // 6, len(at))
        for i, (j, k) in enumerate(at):
            g[..., j] |= p[..., i] << (10 * k)
    out[:, :nb] = g.astype("<u4").view(np.uint8).reshape(H, nb)
    return out


def to_rgb(frame, name, H: int, W: int, matrix: str = "bt709", full_range=False, siting="left"):
    """One packed frame -> ``[H, W, 3]``, uint8 at 8 bits and uint16 in 0 .. 1023 at 10: ``unpack`` for an RGB packing; for a YUV one
    ``unpack``, then yuv.to_rgb / depth10.to_rgb10 on the planes as an I422 / yuv422p10le frame."""
    v = unpack(frame, name, H, W)
    if not is_yuv(name):
        return v
    if bits(name) == 8:
        return _yuv.to_rgb(_yuv.pack(*v, "i420", "422"), "i420", H, W, matrix, full_range, siting, "422")
    return _d10.to_rgb10(_d10.pack10(*v, "i010", "422"), "i010", H, W, matrix, full_range, siting, "422")


def from_rgb(rgb, name, matrix: str = "bt709", full_range=False, siting="left"):
    """``[H, W, 3]`` (uint8 at 8 bits, uint16 with values <= 1023 at 10) -> one packed frame: ``pack`` for an RGB packing; for a YUV one
    yuv.from_rgb / depth10.from_rgb10 as I422 / yuv422p10le, then ``pack`` of its planes."""
    rgb = np.asarray(rgb)
    if rgb.ndim != 3 or rgb.shape[2] != 3 or rgb.dtype != (np.uint8 if bits(name) == 8 else np.uint16):
        raise ValueError(f"{name}: expected [H,W,3] {'uint8' if bits(name) == 8 else 'uint16'}, got {rgb.dtype} {rgb.shape}")
    H, W = rgb.shape[:2]
    check(name, H, W)
    if not is_yuv(name):
        return pack(rgb, name, H, W)
    if bits(name) == 8:
        planes = _yuv.planes(_yuv.from_rgb(rgb, "i420", matrix, full_range, siting, "422"), "i420", H, W, "422")
    else:
        planes = _d10.planes10(_d10.from_rgb10(rgb, "i010", matrix, full_range, siting, "422"), "i010", H, W, "422")
    return pack(planes, name, H, W)
