"""Surfaces without a device (include/pfnl_hip.h SURFACES; pfnl_amd/csrc/surface_geom.h; pfnl_amd/surface.py): the three symbols, the one
argument check as the library makes it and as a plain C++ program makes it from the header, and the numpy side - describe, embed, views,
extract."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from pfnl_amd import _capi, surface

SURFACE_SYMBOLS = ("pfnl_stream_push_surface", "pfnl_stream_pop_surface", "pfnl_op_yuv420_to_rgb_u8_surface")


def _sf(planes, pitches):
    pad = 3 - len(planes)
    return _capi.pfnl_surface((C.c_void_p * 3)(*planes, *([None] * pad)), (C.c_size_t * 3)(*pitches, *([0] * pad)))


# ---- 1. the C-ABI -----------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_typed():
    text = open(os.path.join(ROOT, "include", "pfnl_hip.h")).read()
    declared = set(re.findall(r"\b(pfnl_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    raw = C.CDLL(_capi.LIB_PATH)
    for name in SURFACE_SYMBOLS:
        assert name in declared, f"include/pfnl_hip.h does not declare {name}"
        assert hasattr(raw, name), f"libpfnl_hip.so does not export {name}"
        assert name in _capi.SIGNATURES, f"_capi.SIGNATURES has no {name}"
    assert "typedef struct pfnl_surface" in text
    assert [f[0] for f in _capi.pfnl_surface._fields_] == ["plane", "pitch"]
    assert C.sizeof(_capi.pfnl_surface) == 3 * C.sizeof(C.c_void_p) + 3 * C.sizeof(C.c_size_t)
    assert _capi.load_library().pfnl_version() == 4                             # symbols were added, nothing changed


def test_library_refuses_bad_surfaces_without_a_device():
    lib = _capi.load_library()
    dummy, H, W = C.c_void_p(4096), 16, 24                                      # never dereferenced: every call returns first
    op = lambda sf, fmt, H_, W_, dst=dummy: lib.pfnl_op_yuv420_to_rgb_u8_surface(sf, fmt, 1, 0, H_, W_, dst, None)   # noqa: E731
    good_nv12, good_i420 = _sf([4096, 8192], [W, W]), _sf([4096, 8192, 12288], [W, W // 2, W // 2])
    assert op(None, 1, H, W) == -1 and b"NULL" in lib.pfnl_last_error()         # a NULL surface
    assert op(C.byref(good_nv12), 1, H, W, None) == -1 and b"NULL" in lib.pfnl_last_error()
    for fmt, planes, pitches in ((1, [4096, None], [W, W]), (1, [None, 8192], [W, W]), (2, [4096, 8192, None], [W, W // 2, W // 2]),
                                 (2, [4096, None, 12288], [W, W // 2, W // 2])):
        assert op(C.byref(_sf(planes, pitches)), fmt, H, W) == -1 and b"plane" in lib.pfnl_last_error(), (fmt, planes)
    for fmt, pitches in ((1, [W - 1, W]), (1, [W, W - 1]), (2, [W - 1, W // 2, W // 2]), (2, [W, W // 2 - 1, W // 2]), (2, [W, W // 2, W // 2 - 1]),
                         (2, [W, 0, W // 2])):                                  # one byte short, plane by plane
        assert op(C.byref(_sf([4096, 8192, 12288], pitches)), fmt, H, W) == -1 and b"pitch" in lib.pfnl_last_error(), (fmt, pitches)
    assert op(C.byref(good_nv12), 0, H, W) == -1 and b"fmt" in lib.pfnl_last_error()            # the packed op's own refusals stay
    assert op(C.byref(good_i420), 2, H, W + 1) == -1 and b"even" in lib.pfnl_last_error()
    assert lib.pfnl_op_yuv420_to_rgb_u8_surface(C.byref(good_nv12), 1, 2, 0, H, W, dummy, None) == -1 and b"matrix" in lib.pfnl_last_error()
    index, got = C.c_longlong(7), C.c_int(7)                                    # a NULL session
    assert lib.pfnl_stream_push_surface(None, C.byref(good_nv12), 0) == -1 and b"NULL" in lib.pfnl_last_error()
    assert lib.pfnl_stream_pop_surface(None, C.byref(good_nv12), 0, C.byref(index), C.byref(got)) == -1 and b"NULL" in lib.pfnl_last_error()
    assert (index.value, got.value) == (7, 7)


DRIVER = r"""
#include <cstdio>
#include "surface_geom.h"
int main() {
    alignas(16) char mem[64];
    for (int fmt = -1; fmt <= 6; ++fmt) {
        const pfnl::SurfaceGeom g = pfnl::surface_geom(fmt, 16, 24);
        std::printf("%d %d %d", fmt, g.planes, g.sample_bytes);
        for (int k = 0; k < g.planes; ++k) std::printf(" %d %zu", g.plane[k].rows, g.plane[k].row_bytes);
        pfnl_surface sf{{mem, mem + 2, mem + 4}, {0, 0, 0}};
        for (int k = 0; k < g.planes; ++k) sf.pitch[k] = g.plane[k].row_bytes;
        const char* why = pfnl::surface_refused(&sf, fmt, 16, 24);
        std::printf(" | %s", why ? why : "ok");
        if (g.planes) {
            sf.pitch[g.planes - 1] -= 1;
            why = pfnl::surface_refused(&sf, fmt, 16, 24);
            std::printf(" | %s", why ? why : "ok");
            sf.pitch[g.planes - 1] += 2;                  /* one byte over: fine at 8 bits, odd at 16 */
            why = pfnl::surface_refused(&sf, fmt, 16, 24);
            std::printf(" | %s", why ? why : "ok");
            sf.pitch[g.planes - 1] += 1;
            sf.plane[0] = mem + 1;                        /* an odd pointer */
            why = pfnl::surface_refused(&sf, fmt, 16, 24);
            std::printf(" | %s", why ? why : "ok");
        }
        std::printf("\n");
    }
    return 0;
}
"""


def test_the_check_is_a_host_header_a_plain_cxx_program_can_use(tmp_path):
    """surface_geom.h compiled by the host compiler alone - no hipcc, no HIP headers - gives the table of plane_shapes and the refusals."""
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++") if c and os.path.exists(c)), None)
    assert cxx, "no host C++ compiler (the build's own clang++ is the last candidate)"
    src, exe = tmp_path / "driver.cpp", tmp_path / "driver"
    src.write_text(DRIVER)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "pfnl_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.strip().split("\n")
    assert len(lines) == 8
    names = {v: k for k, v in _capi.PIXEL_FORMATS.items()}
    for line in lines:
        head, *verdicts = [v.strip() for v in line.split("|")]
        fmt, planes, b, *dims = (int(v) for v in head.split())
        if fmt not in names:
            assert planes == 0 and "format" in verdicts[0]
            continue
        shapes = surface.plane_shapes(names[fmt], 16, 24)
        assert planes == len(shapes) and b == shapes[0][2].itemsize
        assert list(zip(dims[0::2], dims[1::2])) == [(rows, n * dt.itemsize) for rows, n, dt in shapes]
        assert verdicts[0] == "ok" and "pitch" in verdicts[1]
        assert (verdicts[2] == "ok" and verdicts[3] == "ok") if b == 1 else ("even" in verdicts[2] and "even" in verdicts[3])


# ---- 2. pfnl_amd/surface.py ---------------------------------------------------------------------------------------------------------------
def test_plane_shapes():
    u8, u16 = np.dtype(np.uint8), np.dtype(np.uint16)
    assert surface.plane_shapes("rgb24", 16, 24) == ((16, 72, u8),)
    assert surface.plane_shapes("rgb10", 16, 24) == ((16, 72, u16),)
    assert surface.plane_shapes("nv12", 16, 24) == ((16, 24, u8), (8, 24, u8))
    assert surface.plane_shapes("p010", 16, 24) == ((16, 24, u16), (8, 24, u16))
    assert surface.plane_shapes("i420", 16, 24) == ((16, 24, u8), (8, 12, u8), (8, 12, u8))
    assert surface.plane_shapes("i010", 16, 24) == ((16, 24, u16), (8, 12, u16), (8, 12, u16))
    for bad in (("yuv420p", 16, 24), ("nv12", 15, 24), ("i420", 16, 23), ("rgb24", 0, 24)):
        with pytest.raises(ValueError):
            surface.plane_shapes(*bad)
    assert surface.plane_shapes("rgb24", 3, 5) == ((3, 15, u8),)                # odd sizes are a 4:2:0 matter


class _FakeTensor:
    """What describe needs of a tensor: data_ptr / stride (in elements) / element_size / shape / dtype."""

    def __init__(self, a, dtype_name=None):
        self._a, self.shape, self.dtype = a, a.shape, "torch." + (dtype_name or a.dtype.name)

    def data_ptr(self):
        return self._a.ctypes.data

    def stride(self):
        return tuple(v // self._a.dtype.itemsize for v in self._a.strides)

    def element_size(self):
        return self._a.dtype.itemsize


def test_describe_accepts_strided_views():
    H, W = 16, 24
    big = np.zeros((H + 8, 64), np.uint8)                                       # a coded surface: 24 rows at a pitch of 64
    chroma = np.zeros((H // 2 + 4, 128), np.uint8)
    ptrs, pitches = surface.describe((big[:H, :W], chroma[:H // 2, :W]), "nv12", H, W)
    assert ptrs == [big.ctypes.data, chroma.ctypes.data] and pitches == [64, 128]
    ptrs, pitches = surface.describe((big[2:2 + H, 6:6 + W], chroma[1:1 + H // 2, 6:6 + W]), "nv12", H, W)   # a window
    assert ptrs == [big.ctypes.data + 2 * 64 + 6, chroma.ctypes.data + 128 + 6] and pitches == [64, 128]
    ptrs, pitches = surface.describe((big[:H, :W], chroma[:H // 2, :W // 2], chroma[:H // 2, 64:64 + W // 2]), "i420", H, W)
    assert ptrs == [big.ctypes.data, chroma.ctypes.data, chroma.ctypes.data + 64] and pitches == [64, 128, 128]
    assert surface.describe((np.zeros((H, W), np.uint8), np.zeros((H // 2, W), np.uint8)), "nv12", H, W)[1] == [W, W]   # packed is a surface too
    pairs = chroma[:H // 2, :W].reshape(H // 2, W // 2, 2)                      # rows split into further axes
    assert surface.describe((big[:H, :W], pairs), "nv12", H, W)[1] == [64, 128]
    rgb = np.zeros((H, 40, 3), np.uint8)
    assert surface.describe((rgb[:, :W],), "rgb24", H, W) == ([rgb.ctypes.data], [120])
    assert surface.describe((rgb.reshape(H, 120)[:, :3 * W],), "rgb24", H, W) == ([rgb.ctypes.data], [120])
    wide = np.zeros((2 * H, 40), np.uint16)
    ptrs, pitches = surface.describe((wide[:H, :W], wide[H:H + H // 2, :W]), "p010", H, W)
    assert ptrs == [wide.ctypes.data, wide.ctypes.data + H * 80] and pitches == [80, 80]
    fake = (_FakeTensor(big[:H, :W]), _FakeTensor(chroma[:H // 2, :W]))          # the tensor protocol: strides in elements
    assert surface.describe(fake, "nv12", H, W) == ([big.ctypes.data, chroma.ctypes.data], [64, 128])
    assert surface.describe((_FakeTensor(wide[:H, :W]), _FakeTensor(wide[H:H + H // 2, :W])), "p010", H, W)[1] == [80, 80]
    sf = surface.as_struct((big[:H, :W], chroma[:H // 2, :W]), "nv12", H, W)
    assert list(sf.plane) == [big.ctypes.data, chroma.ctypes.data, None] and list(sf.pitch) == [64, 128, 0]


def test_describe_refuses_what_is_no_surface():
    H, W = 16, 24
    y, c = np.zeros((H, 64), np.uint8)[:, :W], np.zeros((H // 2, 64), np.uint8)[:, :W]
    assert surface.describe((y, c), "nv12", H, W)[1] == [64, 64]
    bad = [((y,), "nv12"),                                                      # a wrong plane count
           ((y, c, c), "nv12"),
           ((y, c), "i420"),
           ((y, c), "rgb24"),
           ((y.astype(np.int8), c), "nv12"),                                    # a wrong dtype
           ((y.astype(np.uint16), c.astype(np.uint16)), "nv12"),
           ((y, c), "p010"),
           ((y[:, :W - 2], c), "nv12"),                                         # a wrong shape
           ((y[:H - 2], c), "nv12"),
           ((y, c[:, :W // 2]), "nv12"),
           ((np.zeros(H * W, np.uint8), c), "nv12"),                           # flat: no rows
           ((np.zeros((H, 2 * W), np.uint8)[:, ::2], c), "nv12"),               # a last-axis stride of two samples
           ((np.zeros((W, H), np.uint8).T, c), "nv12"),                         # transposed: rows are not contiguous
           ((y[::-1], c), "nv12"),                                              # negative strides
           ((y, c[:, ::-1]), "nv12"),
           ((np.broadcast_to(np.zeros((1, W), np.uint8), (H, W)), c), "nv12"),  # a row stride of 0: below the row
           ((np.lib.stride_tricks.as_strided(np.zeros(H * W, np.uint8), (H, W), (W - 1, 1)), c), "nv12"),   # overlapping rows
           ((_FakeTensor(y, "int8"), _FakeTensor(c)), "nv12"),
           ((object(), c), "nv12")]
    for planes, fmt in bad:
        with pytest.raises(ValueError):
            surface.describe(planes, fmt, H, W)


@pytest.mark.parametrize("fmt", sorted(_capi.PIXEL_FORMATS))
def test_embed_then_extract_is_the_identity_and_the_padding_keeps_the_fill(fmt):
    H, W, fill = 10, 36, 0xC3
    rng = np.random.default_rng(len(fmt) + H)
    shapes = surface.plane_shapes(fmt, H, W)
    planes = [rng.integers(0, 1024 if dt.itemsize == 2 else 256, (rows, n)).astype(dt) for rows, n, dt in shapes]
    rows_bytes = [n * dt.itemsize for _, n, dt in shapes]
    for pitches in (rows_bytes, [r + 2 for r in rows_bytes], [(r + 63) // 64 * 64 + 64 * k for k, r in enumerate(rows_bytes)]):
        bufs = surface.embed(planes, pitches, fill)
        assert [b.shape for b in bufs] == [(rows, p) for (rows, _, _), p in zip(shapes, pitches)] and all(b.dtype == np.uint8 for b in bufs)
        back = surface.extract(bufs, fmt, H, W)
        assert all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in zip(back, planes))
        assert all((b[:, r:] == fill).all() for b, r in zip(bufs, rows_bytes))
        vs = surface.views(bufs, fmt, H, W)                                     # views share the buffers and describe as their pitch
        assert surface.describe(vs, fmt, H, W) == ([b.ctypes.data for b in bufs], list(pitches))
        vs[0][0, 0] = planes[0][0, 0] ^ 1
        assert surface.extract(bufs, fmt, H, W)[0][0, 0] == planes[0][0, 0] ^ 1
    with pytest.raises(ValueError):
        surface.embed(planes, [r - 1 for r in rows_bytes], fill)                # a pitch below the row
    with pytest.raises(ValueError):
        surface.embed(planes, rows_bytes[:-1] + [], fill) if len(planes) > 1 else surface.embed(planes, [], fill)
    with pytest.raises(ValueError):
        surface.views(bufs[:-1], fmt, H, W)


def test_video_stream_has_the_two_methods():
    from pfnl_amd.stream import VideoStream
    assert callable(VideoStream.push_planes) and callable(VideoStream.pop_planes)
    from pfnl_amd import ops
    assert callable(ops.yuv420_to_rgb_surface)
