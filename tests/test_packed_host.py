"""Packed formats without a device: the host rule pfnl_amd/packed.py on literal bytes, its round trips and its composition with the planar
4:2:2 rule (pfnl_amd/yuv.py, pfnl_amd/depth10.py); pfnl_amd/csrc/pack_geom.h compiled as a plain C++17 program and held against packed.py
over every packing, family, depth, chroma format and a few widths; what the library refuses before any HIP call; and the raw pipe of
pfnl_amd/rawvideo.py around a stub session."""
import ctypes as C
import io
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from pfnl_amd import _capi, depth10, rawvideo, stream, surface, yuv
from pfnl_amd import packed as P

NAMES = P.PACKINGS[1:]
RGB8, YUV8, RGB10, YUV10 = ("bgr24", "rgba", "bgra"), ("yuyv422", "uyvy422"), ("x2rgb10", "x2bgr10"), ("y210", "v210")
WIDTHS = (1, 2, 5, 6, 12, 16, 48, 54, 67, 1280, 1920)


def _u32(frame):
    return np.ascontiguousarray(frame).view("<u4")


def _random(name, H, W, seed):
    rng = np.random.default_rng(seed)
    top = 1 << P.bits(name)
    dt = np.uint8 if top == 256 else np.uint16
    if P.is_yuv(name):
        return tuple(rng.integers(0, top, size=s).astype(dt) for s in ((H, W), (H, W // 2), (H, W // 2)))
    return rng.integers(0, top, size=(H, W, 3)).astype(dt)


# ---- known answers on literal bytes ---------------------------------------------------------------------------------------------------------
def test_the_table_is_the_c_abis():
    assert P.PACKINGS == ("none", "bgr24", "rgba", "bgra", "yuyv422", "uyvy422", "x2rgb10", "x2bgr10", "y210", "v210")
    assert _capi.PACKINGS == {n: i for i, n in enumerate(P.PACKINGS)}
    assert [P.packing_id(n) for n in P.PACKINGS] == list(range(10)) and P.packing_id(None) == 0
    for bad in ("yuy2", "V210", 4, ""):
        with pytest.raises(ValueError):
            P.packing_id(bad)
    assert [n for n in NAMES if P.is_yuv(n)] == list(YUV8 + YUV10) and [n for n in NAMES if P.bits(n) == 10] == list(RGB10 + YUV10)
    assert all(P.frame_dtype(n) == np.uint8 for n in NAMES)                     # a frame is its bytes, whatever the unit


def test_v210_words():
    grey = P.pack((np.full((1, 6), 64), np.full((1, 3), 512), np.full((1, 3), 512)), "v210", 1, 6)
    assert grey.shape == (1, 128) and _u32(grey)[0, 0] == 0x20010200             # Cb = 512, Y = 64, Cr = 512
    assert not grey[:, 16:].any()                                                # the row's padding is written 0
    Y, Cb, Cr = np.array([[1, 2, 3, 4, 5, 6]]), np.array([[101, 102, 103]]), np.array([[201, 202, 203]])
    words = [101 | 1 << 10 | 201 << 20,                                          # Cb0 Y0 Cr0
             2 | 102 << 10 | 3 << 20,                                            # Y1 Cb1 Y2
             202 | 4 << 10 | 103 << 20,                                          # Cr1 Y3 Cb2
             5 | 203 << 10 | 6 << 20]                                            # Y4 Cr2 Y5
    group = P.pack((Y, Cb, Cr), "v210", 1, 6)
    assert _u32(group)[0, :4].tolist() == words
    dirty = group.copy()
    _u32(dirty)[0, :4] |= 0xC0000000                                             # bits 31..30 and the padding are ignored on read
    dirty[:, 16:] = 0xFF
    for frame in (group, dirty):
        got = P.unpack(frame, "v210", 1, 6)
        assert all(np.array_equal(g, w) and g.dtype == np.uint16 for g, w in zip(got, (Y, Cb, Cr)))


def test_the_8_bit_pairs_and_the_10_bit_words():
    Y, Cb, Cr = np.array([[10, 20]]), np.array([[30]]), np.array([[40]])
    assert P.pack((Y, Cb, Cr), "yuyv422", 1, 2).tolist() == [[10, 30, 20, 40]]
    assert P.pack((Y, Cb, Cr), "uyvy422", 1, 2).tolist() == [[30, 10, 40, 20]]
    px = np.array([[[1023, 0, 1]]])
    assert _u32(P.pack(px, "x2rgb10", 1, 1))[0, 0] == 0x3FF00001 | 0xC0000000
    assert _u32(P.pack(px, "x2bgr10", 1, 1))[0, 0] == 0x001003FF | 0xC0000000
    y210 = P.pack((np.array([[1023, 0]]), np.array([[1]]), np.array([[512]])), "y210", 1, 2).view("<u2")
    assert y210.tolist() == [[0xFFC0, 1 << 6, 0, 512 << 6]]
    low = y210.copy()
    low |= 0x3F                                                                  # the low six bits are ignored on read
    assert [int(p[0, 0]) for p in P.unpack(low.view(np.uint8), "y210", 1, 2)] == [1023, 1, 512]
    rgb = np.array([[[1, 2, 3]]], np.uint8)
    assert P.pack(rgb, "bgr24", 1, 1).tolist() == [[3, 2, 1]]
    assert P.pack(rgb, "rgba", 1, 1).tolist() == [[1, 2, 3, 255]] and P.pack(rgb, "bgra", 1, 1).tolist() == [[3, 2, 1, 255]]
    for name, frame in (("rgba", [[1, 2, 3, 0]]), ("bgra", [[3, 2, 1, 77]])):   # alpha is ignored on read
        assert P.unpack(np.array(frame, np.uint8), name, 1, 1).tolist() == [[[1, 2, 3]]]
    spare = _u32(P.pack(px, "x2rgb10", 1, 1)) & 0x3FFFFFFF                       # and so are the spare bits of an X2 word
    assert P.unpack(spare.view(np.uint8), "x2rgb10", 1, 1).tolist() == [[[1023, 0, 1]]]


# ---- round trips and the rule -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_unpack_of_pack_over_all_sample_values(name):
    top = 1 << P.bits(name)
    H, W = 4, 6 * ((top // 2 + 5) // 6 + 1)                                      # a chroma plane of H W / 2 >= top samples: every plane holds every value
    v = np.arange(H * W * 3) % top
    samples = (v[:H * W].reshape(H, W), v[:H * W // 2].reshape(H, W // 2), v[::-1][:H * W // 2].reshape(H, W // 2)) if P.is_yuv(name) \
        else v.reshape(H, W, 3)
    for p in (samples if P.is_yuv(name) else (samples,)):
        assert len(np.unique(p)) == top
    frame = P.pack(samples, name, H, W)
    assert frame.shape == P.frame_shape(name, H, W) and frame.dtype == np.uint8 and frame.nbytes == P.frame_bytes(name, H, W)
    got = P.unpack(frame, name, H, W)
    for g, w in zip(got if P.is_yuv(name) else (got,), samples if P.is_yuv(name) else (samples,)):
        assert g.dtype == (np.uint8 if top == 256 else np.uint16) and np.array_equal(g, w)
    assert np.array_equal(P.pack(P.unpack(frame.reshape(-1), name, H, W), name, H, W), frame)      # (a flat buffer is a frame too)
    with pytest.raises(ValueError):
        P.pack(np.full((H, W, 3), top) if not P.is_yuv(name) else (np.full((H, W), top),) + tuple(samples[1:]), name, H, W)
    with pytest.raises(ValueError):
        P.unpack(frame.reshape(-1)[:-1], name, H, W)


@pytest.mark.parametrize("name", YUV8 + YUV10)
def test_to_rgb_and_from_rgb_are_the_planar_rule_behind_the_layout(name):
    H, W = 5, 18
    planes = _random(name, H, W, seed=3)
    frame = P.pack(planes, name, H, W)
    rgb = np.random.default_rng(4).integers(0, 1 << P.bits(name), size=(H, W, 3)).astype(planes[0].dtype)
    for matrix, full in (("bt601", False), ("bt709", True)):
        for siting in yuv.SITINGS:
            if P.bits(name) == 8:
                want = yuv.to_rgb(yuv.pack(*planes, "i420", "422"), "i420", H, W, matrix, full, siting, "422")
                enc = yuv.planes(yuv.from_rgb(rgb, "i420", matrix, full, siting, "422"), "i420", H, W, "422")
            else:
                want = depth10.to_rgb10(depth10.pack10(*planes, "i010", "422"), "i010", H, W, matrix, full, siting, "422")
                enc = depth10.planes10(depth10.from_rgb10(rgb, "i010", matrix, full, siting, "422"), "i010", H, W, "422")
            got = P.to_rgb(frame, name, H, W, matrix, full, siting)
            assert got.dtype == want.dtype and np.array_equal(got, want), (name, matrix, full, siting)
            assert np.array_equal(P.from_rgb(rgb, name, matrix, full, siting), P.pack(enc, name, H, W)), (name, matrix, full, siting)
    assert np.array_equal(P.to_rgb(frame, name, H, W, siting="left"), P.to_rgb(frame, name, H, W, siting="topleft"))   # the horizontal half alone


@pytest.mark.parametrize("name", RGB8 + RGB10)
def test_an_rgb_packing_is_unpack_alone(name):
    H, W = 3, 7
    rgb = _random(name, H, W, seed=5)
    frame = P.from_rgb(rgb, name, "bt601", True, "center")
    assert np.array_equal(frame, P.pack(rgb, name, H, W)) and np.array_equal(P.to_rgb(frame, name, H, W, "bt601", True, "center"), rgb)
    with pytest.raises(ValueError):
        P.from_rgb(rgb.astype(np.uint16 if rgb.dtype == np.uint8 else np.uint8), name)


# ---- sizes and refusals -------------------------------------------------------------------------------------------------------------------
def test_row_and_frame_bytes():
    assert [P.row_bytes(n, 12) for n in NAMES] == [36, 48, 48, 24, 24, 48, 48, 48, 32]
    assert [P.tight_row_bytes(n, 12) for n in NAMES] == [36, 48, 48, 24, 24, 48, 48, 48, 128]
    assert [P.tight_row_bytes("v210", w) for w in (48, 54, 1920, 1280)] == [128, 256, 5120, 3456]
    assert [P.row_bytes("v210", w) for w in (48, 54, 1920)] == [128, 144, 5120]
    assert P.frame_bytes("v210", 1080, 1920) == 1080 * 5120 and P.frame_bytes("v210", 3, 54) == 768 and P.frame_shape("v210", 3, 54) == (3, 256)
    assert P.frame_bytes("yuyv422", 1080, 1920) == 1080 * 1920 * 2 and P.frame_bytes("bgra", 3, 5) == 60 and P.frame_bytes("bgr24", 3, 5) == 45
    assert P.frame_shape("y210", 2, 4) == (2, 16) and P.frame_shape("x2rgb10", 2, 3) == (2, 12)


def test_every_refusal_of_the_table():
    for name in NAMES:
        yuv_side, depth = P.is_yuv(name), P.bits(name)
        assert P.side_refused(name, yuv_side, depth, "422", 12) is None
        assert "family" in P.side_refused(name, not yuv_side, depth, "422", 12)
        assert "depth" in P.side_refused(name, yuv_side, 18 - depth, "422", 12)
        for chroma in ("420", "444"):
            why = P.side_refused(name, yuv_side, depth, chroma, 12)
            assert ("chroma format" in why) if yuv_side else why is None          # an RGB side ignores its chroma format
        assert "width" in P.side_refused(name, yuv_side, depth, "422", 0)
        if yuv_side:
            assert "even width" in P.side_refused(name, yuv_side, depth, "422", 7) or name == "v210"
            for call in (P.check, P.frame_bytes, P.frame_shape):
                with pytest.raises(ValueError):
                    call(name, 2, 7)
        else:
            P.check(name, 1, 7)
        with pytest.raises(ValueError):
            P.check(name, 0, 12)
    for w in (2, 4, 8, 10, 1280):
        assert "multiple of 6" in P.side_refused("v210", True, 10, "422", w)
        with pytest.raises(ValueError, match="multiple of 6"):
            P.frame_bytes("v210", 2, w)
    assert P.side_refused("none", True, 8, "420", 7) is None and P.side_refused(None, False, 10, "444", 1) is None
    with pytest.raises(ValueError):
        P.check("none", 2, 2)


def test_the_keywords_of_open_stream_and_the_one_plane():
    pa = stream.packing_arguments
    assert pa() == (0, 0) and pa("bgra", "rgba", W=5, out_W=20) == (3, 2)
    assert pa("yuyv422", "bgra", "nv12", "rgb24", 8, "422", None, 24, 96) == (4, 3)           # a capture card in, a swap chain out
    assert pa("v210", "y210", "i420", "i010", 10, "422", None, 24, 96) == (9, 8) and pa(None, "x2rgb10", "rgb24", "rgb10") == (0, 6)
    for bad in (("yuyv422",), ("yuyv422", None, "nv12"), ("y210", None, "nv12", None, 8, "422"), (None, "x2rgb10"), (4,), ("yuy2",),
                ("v210", None, "i420", "i010", 10, "422", None, 16), (None, "uyvy422", "rgb24", "i420", 8, "420", "422", 24, 95)):
        with pytest.raises(ValueError):
            pa(*bad)

    class Unready:                                                               # the check comes before anything touches the engine
        class geom:
            scale = 4
    with pytest.raises(ValueError, match="packing"):
        stream.VideoStream(Unready(), 16, 24, 1, packing="yuyv422")
    assert surface.plane_shapes("nv12", 16, 24, "422", "yuyv422") == ((16, 48, np.dtype(np.uint8)),)
    assert surface.plane_shapes("i010", 16, 24, "422", "v210") == ((16, 64, np.dtype(np.uint8)),)
    assert surface.plane_shapes("rgb10", 3, 5, packing="x2bgr10") == ((3, 20, np.dtype(np.uint8)),)
    assert surface.plane_shapes("rgb24", 3, 5, packing=None) == ((3, 15, np.dtype(np.uint8)),)
    for bad in (("rgb24", 16, 24, "420", "yuyv422"), ("nv12", 16, 24, "420", "yuyv422"), ("nv12", 16, 24, "422", "y210"),
                ("i010", 16, 16, "422", "v210")):
        with pytest.raises(ValueError):
            surface.plane_shapes(*bad)
    buf = np.zeros((16, 80), np.uint8)
    (view,) = surface.views([buf], "nv12", 16, 24, "422", "uyvy422")
    assert view.shape == (16, 48) and surface.describe([view], "nv12", 16, 24, "422", "uyvy422") == ([buf.ctypes.data], [80])
    f = stream.packed_frame_argument(np.zeros(16 * 48, np.uint8), "yuyv422", 16, 24)
    assert f.shape == (768,) and stream.packed_frame_argument(np.zeros((16, 128), np.uint8), "v210", 16, 24).shape == (16, 128)
    for bad in (np.zeros((16, 48), np.uint16), np.zeros((16, 47), np.uint8), np.zeros((16, 64), np.uint8)):
        with pytest.raises(ValueError):
            stream.packed_frame_argument(bad, "yuyv422", 16, 24)


# ---- the C++ side -------------------------------------------------------------------------------------------------------------------------
DRIVER = r"""
#include <cstdio>
#include "pack_geom.h"
#include "stream_route.h"
int main() {
    const int widths[] = {1, 2, 5, 6, 12, 16, 48, 54, 67, 1280, 1920};
    for (int pack = -1; pack <= 10; ++pack)
        for (int w : widths) {
            std::printf("G %d %d | %zu %zu %zu\n", pack, w, pfnl::pack_row_bytes(pack, w), pfnl::pack_tight_pitch(pack, w), pfnl::pack_frame_bytes(pack, 3, w));
            for (int yuv = 0; yuv <= 1; ++yuv)
                for (int bits = 8; bits <= 10; bits += 2)
                    for (int chroma = 0; chroma <= 2; ++chroma) {
                        const char* why = pfnl::pack_refused(pack, yuv != 0, bits, chroma, w);
                        std::printf("X %d %d %d %d %d | %s\n", pack, w, yuv, bits, chroma, why ? why : "ok");
                    }
        }
    for (int pack = 1; pack <= 9; ++pack) {
        const pfnl::PackInfo& p = pfnl::PACK_TABLE[pack];
        std::printf("T %d | %d %d %d %d %d\n", pack, (int)p.yuv, p.bits, p.unit_px, p.unit_bytes, p.align);
    }
    // the default argument is PFNL_PACK_NONE, and with it every value is what it was
    for (int fmt = -1; fmt <= 6; ++fmt)
        for (int chroma = 0; chroma <= 2; ++chroma) {
            const pfnl::SurfaceGeom a = pfnl::surface_geom(fmt, 36, 54, chroma), b = pfnl::surface_geom(fmt, 36, 54, chroma, PFNL_PACK_NONE);
            const pfnl::OutRoute r = pfnl::out_route(fmt, 64, 96, 36, 54, chroma), q = pfnl::out_route(fmt, 64, 96, 36, 54, chroma, PFNL_PACK_NONE);
            const char* x = pfnl::route_refused(0, fmt, 36, 54, chroma);
            const char* y = pfnl::route_refused(0, fmt, 36, 54, chroma, PFNL_PACK_NONE);
            std::printf("D %d %d | %d %d %zu %zu %zu | %d %d %d %d %zu %zu %zu %zu | %d\n", fmt, chroma, a.planes, a.sample_bytes,
                        a.plane[0].row_bytes, a.plane[1].row_bytes, a.plane[2].row_bytes, (int)r.runs[0], (int)r.runs[1], (int)r.runs[2], r.last,
                        r.stage_bytes[0], r.stage_bytes[1], r.stage_bytes[2], r.frame_bytes,
                        (int)(a.planes == b.planes && a.sample_bytes == b.sample_bytes && a.plane[1].row_bytes == b.plane[1].row_bytes &&
                              a.plane[0].rows == b.plane[0].rows && r.frame_bytes == q.frame_bytes && r.last == q.last &&
                              r.stage_bytes[2] == q.stage_bytes[2] && x == y));
        }
    // a packed side: one plane; the route's stage 2 and its tight frame
    const int sides[9] = {0, 0, 0, 2, 2, 3, 3, 5, 5};   // an out_fmt of each packing's family and depth
    for (int pack = 1; pack <= 9; ++pack) {
        const pfnl::SurfaceGeom g = pfnl::surface_geom(sides[pack - 1], 36, 54, 1, pack);
        const pfnl::OutRoute r = pfnl::out_route(sides[pack - 1], 64, 96, 36, 54, 1, pack);
        const char* why = pfnl::route_refused(0, sides[pack - 1], 36, 54, 1, pack);
        const char* odd = pfnl::route_refused(0, sides[pack - 1], 36, 55, 1, pack);
        std::printf("P %d | %d %d %d %zu %d | %d %d %zu %zu | %s | %s\n", pack, g.planes, g.sample_bytes, g.plane[0].rows, g.plane[0].row_bytes, g.align,
                    (int)r.runs[2], r.last, r.stage_bytes[2], r.frame_bytes, why ? why : "ok", odd ? odd : "ok");
    }
    const pfnl::SurfaceGeom none = pfnl::surface_geom(0, 36, 54, 0, PFNL_PACK_YUYV);   // a packing its side refuses: no planes
    std::printf("N | %d\n", none.planes);
    return 0;
}
"""


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++") if c and os.path.exists(c)), None)
    assert cxx, "no host C++ compiler (the build's own clang++ is the last candidate)"
    tmp = tmp_path_factory.mktemp("packed")
    src, exe = tmp / "driver.cpp", tmp / "driver"
    src.write_text(DRIVER)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "pfnl_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    text = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    out = {}
    for line in text.strip().split("\n"):
        parts = [p.strip() for p in line.split("|")]
        out.setdefault(parts[0][0], []).append([parts[0][1:].split()] + [p for p in parts[1:]])
    return out


def test_pack_geom_is_packed_py(table):
    chromas = yuv.CHROMAS
    assert len(table["G"]) == 12 * len(WIDTHS) and len(table["X"]) == 12 * len(WIDTHS) * 12
    for (pack, w), sizes in table["G"]:
        pack, w = int(pack), int(w)
        row, tight, frame = (int(v) for v in sizes.split())
        name = P.PACKINGS[pack] if 1 <= pack <= 9 else None
        ok = name is not None and P.side_refused(name, P.is_yuv(name), P.bits(name), "422", w) is None
        assert row == (P.row_bytes(name, w) if ok else 0), (pack, w)
        assert frame == (P.frame_bytes(name, 3, w) if ok else 0), (pack, w)
        assert tight == (P.tight_row_bytes(name, w) if ok or name == "v210" else 0), (pack, w)
    for (pack, w, yuv_side, depth, chroma), verdict in table["X"]:
        pack, w, yuv_side, depth, chroma = int(pack), int(w), int(yuv_side), int(depth), int(chroma)
        if pack in (-1, 10):
            assert "PFNL_PACK_NONE .. PFNL_PACK_V210" in verdict
            continue
        want = P.side_refused(P.PACKINGS[pack], bool(yuv_side), depth, chromas[chroma], w)
        assert verdict == ("ok" if want is None else want), (pack, w, yuv_side, depth, chroma)
    for (pack,), fields in table["T"]:
        assert tuple(int(v) for v in fields.split()) == tuple(int(v) for v in P.TABLE[P.PACKINGS[int(pack)]])


def test_the_default_argument_changes_no_value(table):
    names = {v: k for k, v in _capi.PIXEL_FORMATS.items()}
    assert len(table["D"]) == 8 * 3
    for (fmt, chroma), geom, route, same in table["D"]:
        fmt, chroma = int(fmt), yuv.CHROMAS[int(chroma)]
        planes, width, *rows = (int(v) for v in geom.split())
        r0, r1, r2, last, b0, b1, b2, frame = (int(v) for v in route.split())
        assert same == "1", (fmt, chroma)
        if fmt not in names:
            assert (planes, width, rows, frame) == (0, 0, [0, 0, 0], 0)
            continue
        shapes = surface.plane_shapes(names[fmt], 36, 54, chroma)               # the rule as it stood: the planes of the layout
        assert planes == len(shapes) and width == shapes[0][2].itemsize
        assert rows[:planes] == [n * dt.itemsize for _, n, dt in shapes]
        is_yuv = names[fmt] in _capi.FORMATS_420
        assert (r0, r1, r2, last) == (1, 1, int(is_yuv), 2 if is_yuv else 1)
        assert (b0, b1) == (64 * 96 * 3 * width, 36 * 54 * 3 * width)
        assert b2 == (sum(r * n * dt.itemsize for r, n, dt in shapes) if is_yuv else 0) and frame == (b2 if is_yuv else b1)


def test_a_packed_side_is_one_plane_and_stage_2(table):
    for (pack,), geom, route, verdict, odd in table["P"]:
        name = P.PACKINGS[int(pack)]
        planes, width, rows, row_bytes, align = (int(v) for v in geom.split())
        runs2, last, stage2, frame = (int(v) for v in route.split())
        assert (planes, rows, row_bytes) == (1, 36, P.row_bytes(name, 54)) and width == P.bits(name) // 8 + (P.bits(name) == 10) and align == P.TABLE[name][4]
        assert (runs2, last) == (1, 2) and stage2 == frame == P.frame_bytes(name, 36, 54)
        assert verdict == "ok" and ("even" in odd if P.is_yuv(name) else odd == "ok")   # (the route's own words come first)
    assert table["N"] == [[[], "0"]]


def test_the_library_refuses_before_any_hip_call():
    lib = _capi.load_library()
    dummy = 4096                                                                 # never dereferenced: the hooks return first
    for fn, ten in ((lib.pfnl_op_packed_to_rgb_u8, 0), (lib.pfnl_op_rgb_to_packed_u8, 0), (lib.pfnl_op_packed_to_rgb_u10, 1), (lib.pfnl_op_rgb_to_packed_u10, 1)):
        good = _capi.PACKINGS["v210" if ten else "yuyv422"]
        other = _capi.PACKINGS["yuyv422" if ten else "y210"]
        call = lambda plane=dummy, pitch=256, pack=good, matrix=1, full=0, siting=0, n=1, stride=0, H=2, W=12, rgb=dummy: fn(  # noqa: E731
            plane, pitch, pack, matrix, full, siting, n, stride, H, W, rgb, None)
        assert call(plane=None) == -1 and b"NULL" in lib.pfnl_last_error()
        assert call(rgb=None) == -1 and b"NULL" in lib.pfnl_last_error()
        for pack in (0, 10, -1):
            assert call(pack=pack) == -1 and b"PFNL_PACK_BGR24 .. PFNL_PACK_V210" in lib.pfnl_last_error()
        assert call(pack=other) == -1 and b"depth" in lib.pfnl_last_error()
        assert call(W=11 if not ten else 14) == -1 and (b"multiple of 6" if ten else b"even width") in lib.pfnl_last_error()
        for bad in ({"n": 0}, {"H": 0}, {"W": 0}):
            assert call(**bad) == -1 and b"positive" in lib.pfnl_last_error()
        assert call(matrix=2) == -1 and b"matrix" in lib.pfnl_last_error()
        assert call(full=2) == -1 and call(siting=3) == -1 and call(siting=-1) == -1
        assert call(pitch=(32 if ten else 24) - 4) == -1 and b"pitch" in lib.pfnl_last_error()
        assert call(n=2, stride=256) == -1 and b"frame stride" in lib.pfnl_last_error()
        if ten:
            assert call(plane=dummy + 2) == -1 and b"multiples of" in lib.pfnl_last_error()
            assert call(pitch=258) == -1 and call(n=2, stride=514) == -1 and b"multiples of" in lib.pfnl_last_error()
            assert call(rgb=dummy + 1) == -1 and b"2-byte" in lib.pfnl_last_error()
    assert lib.pfnl_stream_packing(None, 0, 0) == -1 and b"NULL" in lib.pfnl_last_error()
    assert lib.pfnl_stream_packing(None, 4, 99) == -1
    assert lib.pfnl_version() == 4


# ---- the raw pipe ---------------------------------------------------------------------------------------------------------------------------
class _StubSession:
    """open_stream's face without a device: a frame comes back, index and all, after a delay of one push - as uyvy bytes of itself"""

    def __init__(self, log, H, W, batch, **kw):
        log.append(dict(kw, H=H, W=W, batch=batch))
        self.held, self.count, self.closed = [], 0, False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.closed = True

    def _take(self, n):
        out, self.held = self.held[:n], self.held[n:]
        return out

    def push(self, frame):
        assert frame.dtype == np.uint8 and frame.shape == (4, 16)
        self.held.append((self.count, frame[:, ::-1].copy()))
        self.count += 1
        return self._take(len(self.held) - 1)

    def end(self):
        return self._take(len(self.held))


def test_rawvideo_splits_frames_and_delivers_them_in_order():
    H, W = 4, 8
    frames = [np.full((H, 2 * W), 10 + k, np.uint8) + np.arange(2 * W, dtype=np.uint8) for k in range(4)]
    data = b"".join(f.tobytes() for f in frames)
    reader = rawvideo.RawReader(io.BytesIO(data), "yuyv422", H, W)
    assert reader.frame_bytes == 64 and reader.shape == (4, 16)
    log, made, out, err = [], [], io.BytesIO(), io.StringIO()

    def open_stream(H, W, batch=1, **kw):
        made.append(_StubSession(log, H, W, batch, **kw))
        return made[-1]

    assert rawvideo.run(reader, rawvideo.RawWriter(out), open_stream, out_format="uyvy422", batch=2, matrix="bt601", log=err) == 4
    assert made[0].closed and reader.frames == 4 and "4 frames" in err.getvalue()
    assert log[0] == {"H": 4, "W": 8, "batch": 2, "matrix": "bt601", "pixel_format": "i420", "out_format": "i420", "chroma": "422", "out_chroma": "422",
                      "packing": "yuyv422", "out_packing": "uyvy422"}
    assert out.getvalue() == b"".join(f[:, ::-1].tobytes() for f in frames)      # frame by frame, in index order
    with pytest.raises(ValueError, match="frame 2"):                             # a short last frame is refused by its index
        list(rawvideo.RawReader(io.BytesIO(data[:2 * 64 + 5]), "yuyv422", H, W))
    assert len(list(rawvideo.RawReader(io.BytesIO(b""), "yuyv422", H, W))) == 0
    with pytest.raises(ValueError):
        rawvideo.RawReader(io.BytesIO(data), "v210", H, W)                       # a size the packing does not take
    kw = rawvideo.session_keywords
    assert kw("bgra") == {"batch": 1, "pixel_format": "rgb24", "out_format": "rgb24", "packing": "bgra", "out_packing": "bgra"}
    assert kw("v210", "y210", batch=3) == {"batch": 3, "pixel_format": "i420", "out_format": "i010", "in_depth": 10, "chroma": "422", "out_chroma": "422",
                                           "packing": "v210", "out_packing": "y210"}
    assert kw("x2bgr10", "rgba") == {"batch": 1, "pixel_format": "rgb24", "out_format": "rgb24", "in_depth": 10, "packing": "x2bgr10", "out_packing": "rgba"}
    assert kw("yuyv422", "bgra")["out_chroma"] == "420" and kw("rgba", "uyvy422")["out_chroma"] == "422"
    with pytest.raises(ValueError, match="RGB input"):
        kw("yuyv422", "x2rgb10")
    with pytest.raises(ValueError, match="follows"):
        kw("bgra", packing="rgba")
    a = rawvideo.parser().parse_args(["--in-format", "yuyv422", "--size", "270x480", "--synthetic-weights", "0", "--out-format", "uyvy422", "-", "-"])
    assert a.size == (270, 480) and a.matrix == "bt709" and a.siting == "left" and a.batch == 1 and a.out_size is None
