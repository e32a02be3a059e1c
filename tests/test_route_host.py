"""The session's output route without a device (pfnl_amd/csrc/stream_route.h): a plain C++ program that includes only that header prints
out_route for every format and size case and route_refused for every pair of formats, and the table is held against the rule restated
here and against pfnl_amd.stream's frame shapes; the same program runs once more under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from pfnl_amd import _capi
from pfnl_amd.stream import frame_dtype, frame_shapes

SH, SW = 64, 96                                                                 # the network's raster: H = 16, W = 24, scale 4
SIZES = [(0, 0), (36, 54), (37, 55)]                                            # no resize | even | odd (the RGB formats only)
REFUSAL_SIZES = [(36, 54), (37, 54)]

DRIVER = r"""
#include <cstdio>
#include "stream_route.h"
int main() {
    const int sizes[3][2] = {{0, 0}, {36, 54}, {37, 55}};
    for (int fmt = -1; fmt <= 6; ++fmt)
        for (const auto& sz : sizes) {
            if ((sz[0] & 1) && pfnl::is_420(fmt)) continue;
            const pfnl::OutRoute r = pfnl::out_route(fmt, 64, 96, sz[0], sz[1]);
            const pfnl::SurfaceGeom g = pfnl::surface_geom(fmt, r.out_h, r.out_w);
            size_t sum = 0;
            for (int k = 0; k < g.planes; ++k) sum += g.plane[k].rows * g.plane[k].row_bytes;
            std::printf("R %d %d %d | %d %d %d | %d | %zu %zu %zu | %d | %d %d %zu | %zu | %d %d\n", fmt, sz[0], sz[1], (int)r.runs[0],
                        (int)r.runs[1], (int)r.runs[2], r.sample_bytes, r.stage_bytes[0], r.stage_bytes[1], r.stage_bytes[2], r.last, r.out_h,
                        r.out_w, r.frame_bytes, sum, (int)pfnl::is_10bit(fmt), (int)pfnl::is_420(fmt));
        }
    const int refusal_sizes[2][2] = {{36, 54}, {37, 54}};
    for (int in = 0; in <= 5; ++in)
        for (int out = 0; out <= 6; ++out)
            for (const auto& sz : refusal_sizes) {
                const char* why = pfnl::route_refused(in, out, sz[0], sz[1]);
                std::printf("X %d %d %d %d | %s\n", in, out, sz[0], sz[1], why ? why : "ok");
            }
    return 0;
}
"""


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
    """the driver's output, made once: (route lines, refusal lines, the whole text)"""
    text = _build_and_run(tmp_path_factory.mktemp("route"), "driver")
    lines = [line.split("|") for line in text.strip().split("\n")]
    routes = [[[int(v) for v in part.split()[1 if i == 0 else 0:]] for i, part in enumerate(parts)] for parts in lines if parts[0].startswith("R")]
    refusals = [([int(v) for v in parts[0].split()[1:]], parts[1].strip()) for parts in lines if parts[0].startswith("X")]
    return routes, refusals, text


def test_the_route_of_every_format_and_size(table):
    routes, _, _ = table
    names = {v: k for k, v in _capi.PIXEL_FORMATS.items()}
    seen = set()
    for (fmt, oH, oW), runs, (width,), stage_bytes, (last,), (out_h, out_w, frame_bytes), (geom_sum,), (ten, yuv) in routes:
        seen.add((fmt, oH, oW))
        if fmt not in names:                                                    # -1 and 6: no route at all
            assert runs == [0, 0, 0] and width == 0 and stage_bytes == [0, 0, 0] and frame_bytes == 0 == geom_sum and (ten, yuv) == (0, 0)
            continue
        name = names[fmt]
        assert ten == (name in _capi.TEN_BIT_FORMATS) and yuv == (name in _capi.FORMATS_420)
        want_runs = [1, int(oH != 0), int(name in _capi.FORMATS_420)]           # {0}, {0,1}, {0,2} or {0,1,2}
        assert runs == want_runs, (name, oH, oW)
        assert last == max(k for k in range(3) if want_runs[k])
        assert width == (2 if name in ("rgb10", "p010", "i010") else 1) == np.dtype(frame_dtype(name)).itemsize
        assert (out_h, out_w) == ((oH, oW) if oH else (SH, SW))
        want_bytes = [SH * SW * 3 * width, out_h * out_w * 3 * width, out_h * out_w * 3 // 2 * width]
        assert stage_bytes == [b if r else 0 for b, r in zip(want_bytes, want_runs)], (name, oH, oW)
        assert frame_bytes == geom_sum == stage_bytes[last]
        assert frame_bytes == int(np.prod(frame_shapes(name, out_h, out_w)[0])) * width
    rgb = {_capi.PIXEL_FORMATS["rgb24"], _capi.PIXEL_FORMATS["rgb10"]}
    assert seen == {(fmt, *size) for fmt in range(-1, 7) for size in SIZES if size != (37, 55) or fmt in rgb or fmt not in names}


def test_the_refusals_of_every_pair_of_formats(table):
    _, refusals, _ = table
    ten, yuv, rgb10 = (3, 4, 5), (1, 2, 4, 5), 3
    assert [key for key, _ in refusals] == [[i, o, *size] for i in range(6) for o in range(7) for size in REFUSAL_SIZES]
    for (in_fmt, out_fmt, h, w), verdict in refusals:
        if in_fmt in ten:
            assert "10-bit input" in verdict
        elif out_fmt > 5:
            assert verdict != "ok" and "format" in verdict
        elif in_fmt != 0 and out_fmt == rgb10:
            assert "RGB10" in verdict
        elif out_fmt in yuv and (h % 2 or w % 2):
            assert "even" in verdict
        else:
            assert verdict == "ok", (in_fmt, out_fmt, h, w, verdict)
    answers = {tuple(key): verdict for key, verdict in refusals}
    assert all("even" in answers[(0, o, 37, 54)] for o in yuv) and all(answers[(0, o, 37, 54)] == "ok" for o in (0, 3))
    assert "RGB10" in answers[(1, 3, 36, 54)] and answers[(1, 4, 36, 54)] == "ok"


def test_the_driver_is_clean_under_the_sanitizers(table, tmp_path):
    """a stand-alone program: the sanitizers' runtimes are linked into it, nothing is preloaded"""
    assert _build_and_run(tmp_path, "driver_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")) == table[2]
