"""Placement on a canvas without a device: the host rule (pfnl_amd/fit.py place and rects, pfnl_amd/depth10.py place10), open_stream's
keywords (pfnl_amd/stream.py placement_arguments), the library's refusals ahead of any HIP call, and the rectangle check
(pfnl_amd/csrc/stream_route.h place_refused) as a plain C++ program held against the Python rule - once more under the sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from pfnl_amd import _capi, depth10, fit, resize
from pfnl_amd.stream import placement_arguments

FILL = (16, 128, 235)


# ---- 1. rects -----------------------------------------------------------------------------------------------------------------------------
def test_rects_known_answers():
    assert fit.rects(1440, 1920, 1080, 1920, fit="contain") == ((0, 0, 1440, 1920), (0, 240, 1080, 1440))       # 4:3 into 16:9
    assert fit.rects(1440, 1920, 1080, 1920, fit="cover") == ((180, 0, 1080, 1920), (0, 0, 1080, 1920))
    assert fit.rects(2304, 2880, 2160, 3840, fit="contain", sar=(16, 15), g=2) == ((0, 0, 2304, 2880), (0, 480, 2160, 2880))   # PAL x 4
    assert fit.rects(64, 96, 64, 160, fit="contain") == ((0, 0, 64, 96), (0, 32, 64, 96))
    assert fit.rects(64, 96, 36, 54) == ((0, 0, 64, 96), (0, 0, 36, 54))                                        # no fit: the stretch
    assert fit.rects(64, 96, 36, 54, crop=(8, 12, 48, 72)) == ((8, 12, 48, 72), (0, 0, 36, 54))
    for bad in [dict(fit="stretch"), dict(sar=(0, 1)), dict(sar=3), dict(g=3), dict(crop=(0, 0, 65, 96)), dict(crop=(0, 0, 0, 96)), dict(crop=(1, 2, 3))]:
        with pytest.raises(ValueError):
            fit.rects(64, 96, 36, 54, **bad)
    with pytest.raises(ValueError, match="src -> dst"):                         # the pair breaks the per-axis limits
        fit.rects(64, 96, 8, 8, fit="contain")


def test_rects_properties():
    rng = np.random.default_rng(2024)
    seen = {"contain": 0, "cover": 0}
    for _ in range(600):
        sH, sW, oH, oW = (int(v) for v in rng.integers(16, 400, 4))
        g = int(rng.integers(1, 3))
        oH, oW = oH // g * g, oW // g * g
        sar = (int(rng.integers(1, 5)), int(rng.integers(1, 5))) if rng.integers(0, 2) else (1, 1)
        crop = None
        if rng.integers(0, 2):
            ch, cw = int(rng.integers(8, sH + 1)), int(rng.integers(8, sW + 1))
            crop = (int(rng.integers(0, sH - ch + 1)), int(rng.integers(0, sW - cw + 1)), ch, cw)
        for mode in ("contain", "cover"):
            try:
                src, dst = fit.rects(sH, sW, oH, oW, crop, mode, sar, g)
            except ValueError as e:
                assert "src -> dst" in str(e)                                   # only the resampler's limits refuse these
                continue
            seen[mode] += 1
            cy, cx, ch, cw = crop or (0, 0, sH, sW)
            (sy, sx, sh, sw), (dy, dx, dh, dw) = src, dst
            assert 0 <= dy and dy + dh <= oH and 0 <= dx and dx + dw <= oW and dh >= 1 and dw >= 1
            assert (dy == 0 and dh == oH) or (dx == 0 and dw == oW)             # both ends of at least one axis
            assert all(v % g == 0 for v in dst)
            assert abs(dy - (oH - dh - dy)) <= g and abs(dx - (oW - dw - dx)) <= g   # centred to within g
            assert cy <= sy and sy + sh <= cy + ch and cx <= sx and sx + sw <= cx + cw and sh >= 1 and sw >= 1
            if mode == "contain":
                assert src == (cy, cx, ch, cw)
            else:
                assert dst == (0, 0, oH, oW) and (sh == ch or sw == cw)
                assert abs((cy + ch - sy - sh) - (sy - cy)) <= 1 and abs((cx + cw - sx - sw) - (sx - cx)) <= 1
    assert seen["contain"] > 200 and seen["cover"] > 200


# ---- 2. place and place10 -----------------------------------------------------------------------------------------------------------------
def _frames(depth):
    rng = np.random.default_rng(5 + depth)
    if depth == 8:
        return rng.integers(0, 256, (64, 96, 3), np.uint8), rng.integers(0, 256, (64, 96, 3), np.uint8)
    return rng.integers(0, 1024, (64, 96, 3), np.uint16), rng.integers(0, 1024, (64, 96, 3), np.uint16)


@pytest.mark.parametrize("depth", [8, 10])
def test_place_properties(depth):
    place, rs, colour = (fit.place, resize.resize, FILL) if depth == 8 else (depth10.place10, depth10.resize10, depth10.fill10(FILL))
    if depth == 10:
        assert colour == tuple((v << 2) | (v >> 6) for v in FILL) == (64, 514, 943)
        assert depth10.fill10((0, 255, 1)) == (0, 1023, 4)
    a, b = _frames(depth)
    assert np.array_equal(place(a, 36, 54), rs(a, 36, 54))                       # src and dst whole: the resize
    assert np.array_equal(place(a, 36, 54, (0, 0, 64, 96), (0, 0, 36, 54), FILL), rs(a, 36, 54))
    src, dst = (8, 12, 48, 72), (2, 9, 32, 47)
    got = place(a, 37, 64, src, dst, FILL)
    assert got.dtype == a.dtype and got.shape == (37, 64, 3)
    outside = np.ones((37, 64), bool)
    outside[2:34, 9:56] = False
    assert (got[outside] == np.array(colour)).all()                              # every sample outside dst is the fill,
    assert np.array_equal(place(b, 37, 64, src, dst, FILL)[outside], got[outside])   # whatever the frame
    assert np.array_equal(got[2:34, 9:56], rs(a[8:56, 12:84], 32, 47))           # the composition: clamping at the edges of src
    c = b.copy()
    c[8:56, 12:84] = a[8:56, 12:84]                                              # other pixels outside src: nothing changes
    assert not np.array_equal(c, a) and np.array_equal(place(c, 37, 64, src, dst, FILL), got)
    assert not np.array_equal(got[2:34, 9:56], rs(a, 64, 96 * 47 // 72 + 1)[:32, :47])   # (and it is no window of the frame's own resize)
    flat = np.empty_like(a)
    flat[:] = np.array([3, 200, 77], a.dtype)
    flat[:8], flat[56:], flat[:, :12], flat[:, 84:] = 255, 0, 255, 0              # (what surrounds src is not flat)
    assert (place(flat, 37, 64, src, dst, FILL)[2:34, 9:56] == np.array([3, 200, 77])).all()   # a flat rectangle stays flat
    paste = place(a, 80, 128, None, (8, 16, 64, 96), FILL)                       # equal sizes: the bytes, unchanged
    assert np.array_equal(paste[8:72, 16:112], a) and (paste[:8] == np.array(colour)).all() and (paste[:, 112:] == np.array(colour)).all()
    assert np.array_equal(place(a, 32, 48, (16, 24, 32, 48)), a[16:48, 24:72])   # crop only
    assert (place(a, 80, 128, None, (8, 16, 64, 96))[:8] == 0).all()             # the default fill is black
    for bad in [dict(src=(0, 0, 65, 96)), dict(src=(-1, 0, 8, 96)), dict(dst=(0, 0, 37, 65)), dict(dst=(0, 60, 8, 8)), dict(dst=(0, 0, 0, 8)),
                dict(src=(0, 0, 64, 96), dst=(0, 0, 15, 64)), dict(src=(0, 0, 8, 8), dst=(0, 0, 17, 8)), dict(fill=(0, 0, 256)), dict(fill=(1, 2))]:
        with pytest.raises(ValueError):
            place(a, 37, 64, **bad)
    with pytest.raises(ValueError):
        place(a.astype(np.int32), 37, 64)


def test_yuv_bars_follow_the_existing_rule():
    """nothing new is defined for 4:2:0: the canvas is converted like any frame, so black bars are Y 16 / 64 and chroma 128 / 512"""
    from pfnl_amd import yuv
    a, _ = _frames(8)
    nv12 = yuv.from_rgb(fit.place(a, 64, 160, None, (0, 32, 64, 96)), "nv12", "bt601")
    assert (nv12[:64, :30] == 16).all() and (nv12[64:, :30] == 128).all()
    a10, _ = _frames(10)
    i010 = depth10.from_rgb10(depth10.place10(a10, 64, 160, None, (0, 32, 64, 96)), "i010", "bt709")
    assert (i010[:64, :30] == 64).all() and (i010.reshape(-1)[64 * 160:].reshape(2, 32, 80)[:, :, :15] == 512).all()


# ---- 3. open_stream's keywords ------------------------------------------------------------------------------------------------------------
def test_placement_arguments():
    pa = placement_arguments
    assert pa(None, 64, 96) == (0, 0, None, None, (0, 0, 0))                     # all defaults: no call
    assert pa((36, 54), 64, 96) == (36, 54, None, None, (0, 0, 0))               # a size alone: pfnl_stream_resize, as ever
    assert pa((64, 160), 64, 96, fit="contain") == (64, 160, (0, 0, 64, 96), (0, 32, 64, 96), (0, 0, 0))
    assert pa((36, 96), 64, 96, "nv12", crop=(8, 0, 48, 96)) == (36, 96, (8, 0, 48, 96), (0, 0, 36, 96), (0, 0, 0))
    assert pa((48, 128), 64, 96, "p010", place=(6, 16, 36, 54), fill=FILL) == (48, 128, (0, 0, 64, 96), (6, 16, 36, 54), FILL)
    assert pa(None, 64, 96, crop=(8, 0, 48, 96)) == (48, 96, (8, 0, 48, 96), (0, 0, 48, 96), (0, 0, 0))   # the crop at its own size
    assert pa((1080, 1920), 1440, 1920, fit="contain")[3] == (0, 240, 1080, 1440)
    assert pa((1088, 1920), 1080, 1920, "nv12", place=(0, 0, 1080, 1920))[2:4] == ((0, 0, 1080, 1920), (0, 0, 1080, 1920))
    assert pa((2160, 3840), 2304, 2880, "p010", fit="contain", sar=(16, 15))[3] == (0, 480, 2160, 2880)
    with pytest.raises(ValueError, match="exclude"):
        pa((64, 160), 64, 96, fit="contain", place=(0, 32, 64, 96))
    with pytest.raises(ValueError, match="dst"):                                 # a rectangle outside its raster
        pa((64, 160), 64, 96, place=(0, 100, 64, 96))
    with pytest.raises(ValueError, match="src"):
        pa((64, 160), 64, 96, crop=(0, 0, 65, 96), fit="contain")
    with pytest.raises(ValueError, match="src -> dst"):                          # a ratio outside the limits
        pa((64, 160), 64, 96, place=(0, 0, 8, 8))
    with pytest.raises(ValueError, match="even"):                                # an odd canvas with nv12
        pa((37, 54), 64, 96, "nv12", fit="contain")
    with pytest.raises(ValueError, match="even"):
        pa(None, 64, 96, "nv12", crop=(0, 0, 33, 96))
    for bad in [dict(fit="fill"), dict(sar=(16, 15)), dict(sar=(0, 1), fit="cover"), dict(fill=(0, 0, 300)), dict(place=(0, 0, 8)), dict(crop="top")]:
        with pytest.raises(ValueError):
            pa((64, 160), 64, 96, **bad)
    assert pa((64, 160), 64, 96, "rgb24", None, "contain", None, (1, 1), (1, 2, 3))[4] == (1, 2, 3)   # the keywords' order


# ---- 4. the library without a device ------------------------------------------------------------------------------------------------------
def test_the_library_refuses_before_any_hip_call():
    lib = _capi.load_library()
    R = _capi.rect_arg
    assert lib.pfnl_version() == 4
    assert lib.pfnl_stream_place(None, 48, 128, None, None, None) == -1 and b"NULL" in lib.pfnl_last_error()
    assert lib.pfnl_stream_place(None, 0, 0, None, None, None) == -1 and b"NULL" in lib.pfnl_last_error()
    dummy = C.c_void_p(16)                                                       # never dereferenced: the hooks return first
    for hook, ctype in ((lib.pfnl_op_resize_place_u8, C.c_uint8), (lib.pfnl_op_resize_place_u10, C.c_uint16)):
        fill = (ctype * 3)(16, 128, 235)
        call = lambda src, dst, i=dummy, o=dummy, n=1, f=fill, H=64, W=96, oH=64, oW=160: (  # noqa: E731
            hook(i, n, H, W, oH, oW, R(src), R(dst), f, o, None), lib.pfnl_last_error())
        assert call(None, (0, 32, 64, 96), i=None) == (-1, b"NULL argument")
        status, msg = call(None, (0, 32, 64, 96), o=None)
        assert status == -1 and b"NULL" in msg
        status, msg = call(None, (0, 32, 64, 96), n=0)
        assert status == -1 and b"n >= 1" in msg
        for src in [(0, 0, 65, 96), (1, 0, 64, 96), (0, 90, 8, 8), (-1, 0, 8, 8), (0, 0, 0, 96), (0, 0, 2 ** 31 - 1, 96), (2 ** 31 - 1, 0, 8, 8)]:
            status, msg = call(src, (0, 32, 64, 96))
            assert status == -1 and b"src" in msg and b"dst" not in msg, (src, msg)
        for dst in [(0, 65, 64, 96), (1, 0, 64, 96), (0, 0, 64, 161), (0, -2, 64, 96), (0, 0, 64, 0), (0, 2 ** 31 - 1, 64, 96)]:
            status, msg = call(None, dst)
            assert status == -1 and b"dst" in msg and b"src" not in msg, (dst, msg)
        for src, dst in [(None, (0, 0, 15, 96)), (None, (0, 0, 64, 23)), ((0, 0, 8, 8), (0, 0, 17, 8)), ((0, 0, 8, 8), (0, 0, 8, 17))]:
            status, msg = call(src, dst)
            assert status == -1 and b"src" in msg and b"dst" in msg and b"quarter" in msg, (src, dst, msg)
        for size in [dict(H=0), dict(W=20000), dict(oH=-4), dict(oW=16385)]:
            status, msg = call((0, 0, 8, 8), (0, 0, 8, 8), **size)
            assert status == -1 and (b"src" in msg or b"dst" in msg), (size, msg)
        status, msg = call(None, None, oH=8)                                     # whole onto whole: the resize's own refusal
        assert status == -1 and b"resize" in msg
    status = lib.pfnl_op_resize_place_u10(dummy, 1, 64, 96, 64, 160, None, R((0, 32, 64, 96)), (C.c_uint16 * 3)(0, 1024, 0), dummy, None)
    assert status == -1 and b"fill" in lib.pfnl_last_error() and b"1023" in lib.pfnl_last_error()
    status = lib.pfnl_op_resize_place_u10(C.c_void_p(17), 1, 64, 96, 64, 160, None, R((0, 32, 64, 96)), None, dummy, None)
    assert status == -1 and b"aligned" in lib.pfnl_last_error()


# ---- 5. place_refused as a stand-alone program ----------------------------------------------------------------------------------------------
SH, SW = 64, 96
CANVASES = [(64, 160), (37, 55), (16384, 16384), (16385, 8), (0, 8)]
RECTS = [(0, 0, 64, 96), (8, 12, 48, 72), (0, 0, 65, 96), (1, 0, 64, 96), (0, 90, 8, 8), (-1, 0, 8, 8), (0, 0, 0, 96), (0, 0, 16, 24), (0, 0, 15, 24),
         (0, 0, 37, 55), (0, 0, 64, 160), (24, 8, 16, 24), (10, 0, 3, 96), (20, 0, 1, 96), (0, 0, 2147483647, 8), (2147483647, 0, 8, 8),
         (0, 2147483647, 8, 2147483647), (0, 0, 16384, 16384), (0, 0, 128, 193), (0, 0, 129, 192)]

DRIVER = r"""
#include <cstdio>
#include "stream_route.h"
int main() {
    const int canvases[%d][2] = {%s};
    const pfnl_rect rects[%d] = {%s};
    for (const auto& cv : canvases)
        for (const pfnl_rect& src : rects)
            for (const pfnl_rect& dst : rects) {
                const char* why = pfnl::place_refused(%d, %d, cv[0], cv[1], src, dst);
                std::printf("%%d %%d | %%d %%d %%d %%d | %%d %%d %%d %%d | %%s\n", cv[0], cv[1], src.y, src.x, src.h, src.w, dst.y, dst.x, dst.h, dst.w,
                            why ? why : "ok");
            }
    const pfnl_rect one{0, 0, 1, 1};
    std::printf("S %%s\n", pfnl::place_refused(0, 96, 8, 8, one, one));
    std::printf("S %%s\n", pfnl::place_refused(64, 16385, 8, 8, one, one));
    return 0;
}
""" % (len(CANVASES), ", ".join("{%d, %d}" % c for c in CANVASES), len(RECTS), ", ".join("{%d, %d, %d, %d}" % r for r in RECTS), SH, SW)


def _compiler():
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++") if c and os.path.exists(c)), None)
    assert cxx, "no host C++ compiler (the build's own clang++ is the last candidate)"
    return cxx


def _build_and_run(tmp_path, name, extra=()):
    src, exe = tmp_path / "driver.cpp", tmp_path / name
    src.write_text(DRIVER)
    subprocess.run([_compiler(), "-std=c++17", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "pfnl_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return _build_and_run(tmp_path_factory.mktemp("place"), "driver")


def test_place_refused_agrees_with_the_python_rule(table):
    lines = table.strip().split("\n")
    cases = [line for line in lines if not line.startswith("S")]
    assert len(cases) == len(CANVASES) * len(RECTS) ** 2
    verdicts = {"ok": 0, "src": 0, "dst": 0, "ratio": 0, "canvas": 0}
    it = iter(cases)
    for canvas in CANVASES:
        for src in RECTS:
            for dst in RECTS:
                head, s, d, verdict = (part.strip() for part in next(it).split("|"))
                assert [int(v) for v in head.split()] == list(canvas) and tuple(int(v) for v in s.split()) == src
                assert tuple(int(v) for v in d.split()) == dst
                try:
                    fit.check_rects(SH, SW, *canvas, src, dst)
                    want = "ok"
                except ValueError as e:
                    want = str(e)
                assert (verdict == "ok") == (want == "ok"), (canvas, src, dst, verdict, want)
                if verdict == "ok":
                    resize.check_limits(src[2], dst[2])                         # and the resampler takes what was let through
                    resize.check_limits(src[3], dst[3])
                    verdicts["ok"] += 1
                    continue
                assert verdict.startswith("place: ")
                kind = ("canvas" if "canvas sizes" in want else "ratio" if "src -> dst" in want else "src" if "src (" in want else "dst")
                verdicts[kind] += 1
                if kind == "canvas":
                    assert "canvas" in verdict
                elif kind == "ratio":
                    assert "src." in verdict and "dst." in verdict and "quarter" in verdict
                else:
                    assert kind in verdict and {"src": "dst", "dst": "src"}[kind] not in verdict, (src, dst, verdict)
    assert all(v > 0 for v in verdicts.values()), verdicts
    assert [line for line in lines if line.startswith("S")] == ["S place: the raster src lies in must be 1 .. 16384 a side"] * 2


def test_the_driver_is_clean_under_the_sanitizers(table, tmp_path):
    """a stand-alone program: the sanitizers' runtimes are linked into it, nothing is preloaded"""
    assert _build_and_run(tmp_path, "driver_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")) == table
