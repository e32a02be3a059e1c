"""The session's input route without a device (pfnl_amd/csrc/stream_route.h InRoute): a plain C++ program that includes only that header
prints in_route for every layout, depth, chroma format, packing and two sizes, and the table is held against pfnl_amd.stream's frame
shapes, pfnl_amd.surface's planes, pfnl_amd.packed's frames and the header's own refusals; the same program runs once more under the
address and undefined-behaviour sanitizers."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from pfnl_amd import _capi, packed, surface
from pfnl_amd.stream import frame_dtype, frame_shapes, pushed_format
from test_route_host import _compiler                                          # (the output route's test: the same host compiler)

SIZES = [(16, 24), (8, 50)]                  # v210 takes 24 (rows of 64 bytes at a tight pitch of 128) and refuses 50 (tight pitch 256: above any row)
LAYOUTS, DEPTHS, CHROMAS = ("rgb24", "nv12", "i420"), (8, 10), ("420", "422", "444")
KINDS = {"none": 0, "copy": 1, "420": 2, "chroma": 3, "pack": 4}

DRIVER = r"""
#include <cstdio>
#include "stream_route.h"
int main() {
    const int sizes[2][2] = {{16, 24}, {8, 50}};
    const int twin[3] = {PFNL_PIX_RGB10, PFNL_PIX_P010, PFNL_PIX_I010};   // the layout's name at a depth of 10
    for (int fmt = PFNL_PIX_RGB24; fmt <= PFNL_PIX_I420; ++fmt)
        for (int depth = 8; depth <= 10; depth += 2)
            for (int chroma = PFNL_CHROMA_420; chroma <= PFNL_CHROMA_444; ++chroma)
                for (int pack = PFNL_PACK_NONE; pack <= PFNL_PACK_V210; ++pack)
                    for (const auto& sz : sizes) {
                        const pfnl::InRoute r = pfnl::in_route(fmt, depth, chroma, pack, sz[0], sz[1]);
                        const int pushed = depth == 10 ? twin[fmt] : fmt;
                        const bool geom = pfnl::surface_geom(pushed, sz[0], sz[1], chroma, pack).planes != 0;
                        const bool packs = !pfnl::pack_refused(pack, pfnl::is_yuv(fmt), depth, chroma, sz[1]);
                        std::printf("I %d %d %d %d %d %d | %d %d %d %d | %d %zu %d %zu %d %zu | %zu %zu %zu | %zu %zu %zu | %d %d\n", fmt, depth, chroma,
                                    pack, sz[0], sz[1], r.kind, r.fmt, r.geom.planes, r.sample_bytes, r.geom.plane[0].rows, r.geom.plane[0].row_bytes,
                                    r.geom.plane[1].rows, r.geom.plane[1].row_bytes, r.geom.plane[2].rows, r.geom.plane[2].row_bytes, r.pitch[0],
                                    r.pitch[1], r.pitch[2], r.frame_bytes, r.staging_bytes, r.ring_bytes, (int)geom, (int)packs);
                    }
    const pfnl::InRoute bad[3] = {pfnl::in_route(PFNL_PIX_RGB10, 8, 0, 0, 16, 24), pfnl::in_route(-1, 8, 0, 0, 16, 24), pfnl::in_route(0, 12, 0, 0, 16, 24)};
    for (const pfnl::InRoute& r : bad) std::printf("B %d %zu %zu %zu\n", r.kind, r.frame_bytes, r.staging_bytes, r.ring_bytes);
    return 0;
}
"""


def _build_and_run(tmp_path, name, extra=()):
    src, exe = tmp_path / "driver.cpp", tmp_path / name
    src.write_text(DRIVER)
    subprocess.run([_compiler(), "-std=c++17", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "pfnl_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """the driver's output, made once: ({key: the numbers behind it}, the three answers to no layout at all, the whole text)"""
    text = _build_and_run(tmp_path_factory.mktemp("input_route"), "driver")
    rows, bad = {}, []
    for line in text.strip().split("\n"):
        parts = [[int(v) for v in part.split()[1 if i == 0 else 0:]] for i, part in enumerate(line.split("|"))]
        if line.startswith("I"):
            rows[tuple(parts[0])] = parts[1:]
        else:
            bad.append(parts[0])
    return rows, bad, text


def test_every_combination_has_its_row(table):
    rows, bad, _ = table
    want = {(_capi.PIXEL_FORMATS[f], d, _capi.CHROMA_FORMATS[c], p, h, w)
            for f in LAYOUTS for d in DEPTHS for c in CHROMAS for p in range(len(packed.PACKINGS)) for h, w in SIZES}
    assert set(rows) == want and len(want) == 3 * 2 * 3 * 10 * 2
    assert bad == [[0, 0, 0, 0]] * 3                                            # a 10-bit name, no format, no such depth: no route


def test_the_route_of_every_input_setting(table):
    rows, _, _ = table
    routed = 0
    for layout in LAYOUTS:
        for depth in DEPTHS:
            for chroma in CHROMAS:
                for pack, packing in enumerate(packed.PACKINGS):
                    for H, W in SIZES:
                        key = (_capi.PIXEL_FORMATS[layout], depth, _capi.CHROMA_FORMATS[chroma], pack, H, W)
                        (kind, fmt, planes, width), geom, pitch, (frame, staging, ring), (geom_ok, pack_ok) = rows[key]
                        is_yuv = layout != "rgb24"
                        refused = packed.side_refused(packing, is_yuv, depth, chroma, W)    # the rule restated on the host
                        assert bool(pack_ok) == (refused is None) == bool(geom_ok), key   # pack_refused / surface_geom: the header's own
                        if refused is not None:                                 # no route: kind "none", zero sizes
                            assert kind == KINDS["none"] and planes == 0 and geom == [0] * 6 and pitch == [0] * 3
                            assert (frame, staging, ring) == (0, 0, 0), key
                            continue
                        routed += 1
                        name = pushed_format(layout, depth)
                        item = np.dtype(frame_dtype(name)).itemsize
                        assert fmt == _capi.PIXEL_FORMATS[name] and width == item == (2 if depth == 10 else 1)
                        assert ring == H * W * 3 * item
                        if pack:
                            assert kind == KINDS["pack"] and planes == 1
                            assert geom == [H, packed.row_bytes(packing, W), 0, 0, 0, 0]
                            assert pitch == [packed.tight_row_bytes(packing, W), 0, 0] and pitch[0] >= geom[1]
                            assert frame == packed.frame_bytes(packing, H, W) == int(np.prod(packed.frame_shape(packing, H, W)))
                        else:
                            shapes = surface.plane_shapes(name, H, W, chroma)
                            assert planes == len(shapes) == {"rgb24": 1, "nv12": 2, "i420": 3}[layout]
                            want = [v for rows_, n, dt in shapes for v in (rows_, n * dt.itemsize)]
                            assert geom == want + [0] * (6 - len(want)), key
                            assert pitch == [n * dt.itemsize for _, n, dt in shapes] + [0] * (3 - planes)   # tight: a row's own bytes
                            assert frame == int(np.prod(frame_shapes(name, H, W, chroma)[0])) * item, key
                            assert kind == (KINDS["copy"] if not is_yuv else KINDS["420"] if chroma == "420" else KINDS["chroma"])
                        assert staging == (0 if kind == KINDS["copy"] else frame)   # 0 exactly for planar RGB
                        assert (staging == 0) == (layout == "rgb24" and not pack)
    v210 = packed.PACKINGS.index("v210")
    at = lambda H, W: rows[(_capi.PIXEL_FORMATS["i420"], 10, _capi.CHROMA_FORMATS["422"], v210, H, W)]   # noqa: E731
    assert at(16, 24)[2][0] == 128 > at(16, 24)[1][1] == 64 and at(16, 24)[3][0] == 16 * 128
    assert at(8, 50)[0][0] == KINDS["none"] and packed.tight_row_bytes("v210", 50) == 256
    # per size: planes at every layout, depth and chroma format | an RGB packing of either depth at any chroma format (3 + 2 packings) | a YUV
    # packing of either depth in both YUV layouts at 4:2:2 (2 + 2 packings); less v210 at W = 50 in both layouts
    assert routed == 2 * (3 * 2 * 3 + (3 + 2) * 3 + (2 + 2) * 2) - 2


def test_the_driver_is_clean_under_the_sanitizers(table, tmp_path):
    """a stand-alone program: the sanitizers' runtimes are linked into it, nothing is preloaded"""
    assert _build_and_run(tmp_path, "driver_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")) == table[2]
