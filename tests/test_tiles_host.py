"""The tiled forward's device-free side: the rule (pfnl_amd/tiles.py: axis, grid, runs, split, assemble, forward_tiled, check), the same
geometry in C++ (pfnl_amd/csrc/tile_geom.h through a stand-alone program, plain and under the sanitizers, and through pfnl_tile_axis),
and the argument checks of the C-ABI, the engine and the session that need no device (include/pfnl_hip.h TILES)."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from pfnl_amd import _capi, synth, tiles
from pfnl_amd.spec import PFNLGeometry

ABS_TOL = 5e-5                                                                  # the project's forward bound (tests/test_gpu_forward.py)
N_MAX = 64


def _legal(n_max=N_MAX):
    """every even n <= n_max with every legal (t, p): the unsplit axes once each (t = 0, t = n, t = n + 2), the split ones with every p"""
    for n in range(2, n_max + 1, 2):
        for t in (0, n, n + 2):
            yield n, t, 0
        yield n, 0, 5                                                           # (pad is not looked at where the axis is not split)
        for t in range(2, n, 2):
            for p in range(0, (t + 1) // 2):
                if 2 * p < t:
                    yield n, t, p


def test_axis_invariants():
    seen = 0
    for n, t, p in _legal():
        ax = tiles.axis(n, t, p)
        seen += 1
        if t == 0 or t >= n:
            assert ax == [(0, 0, n)]
            continue
        step = t - 2 * p
        assert len(ax) == -(-(n - 2 * p) // step) >= 2
        owned = []
        for i, (o, a, b) in enumerate(ax):
            assert o % 2 == 0 and 0 <= o and o + t <= n, (n, t, p, ax)          # even origins, inside the frame
            assert o <= a < b <= o + t, (n, t, p, ax)                           # non-empty, inside its tile
            lo, hi = (0 if o == 0 else p), (0 if o + t == n else p)             # p from each tile edge that is not a frame edge
            assert a - o >= lo and o + t - b >= hi, (n, t, p, ax)
            owned += list(range(a, b))
        assert owned == list(range(n)), (n, t, p, ax)                           # a partition, in order
        # count is minimal: k tiles whose interior margins are p own at most k t - 2 (k - 1) p samples
        k = len(ax) - 1
        assert k * t - 2 * (k - 1) * p < n, (n, t, p, ax)
    assert seen > 1000


def test_axis_known_answers():
    assert tiles.axis(36, 16, 2) == [(0, 0, 14), (12, 14, 22), (20, 22, 36)]
    assert tiles.axis(34, 14, 3) == [(0, 0, 11), (8, 11, 19), (16, 19, 23), (20, 23, 34)]
    assert tiles.axis(20, 12, 2) == [(0, 0, 10), (8, 10, 20)]
    assert tiles.grid(20, 36, (12, 16, 2)) == (12, 16, tiles.axis(20, 12, 2), tiles.axis(36, 16, 2))
    assert tiles.grid(20, 36, (0, 16, 2))[:2] == (20, 16) and tiles.grid(20, 36, (12, 40))[:2] == (12, 36)
    assert tiles.runs(12, 0) == [(0, 12)] and tiles.runs(12, 4) == [(0, 4), (4, 4), (8, 4)]
    assert tiles.runs(12, 5) == [(0, 5), (5, 5), (10, 2)] and tiles.runs(3, 7) == [(0, 3)]
    assert tiles.tiling((8, 12)) == (8, 12, 0, 0) and tiles.tiling([8, 12, 2]) == (8, 12, 2, 0) and tiles.tiling((8, 12, 2, 3)) == (8, 12, 2, 3)


BAD = [(21, 36, (12, 16, 2)), (20, 35, (12, 16, 2)), (0, 36, (12, 16, 2)), (20, 36, (11, 16, 2)), (20, 36, (12, 15, 2)),
       (20, 36, (12, 16, 6)), (20, 36, (12, 16, 8)), (20, 36, (-2, 16, 0)), (20, 36, (12, 16, -1)), (20, 36, (12, 16, 2, -1)),
       (20, 36, (40, 16, 8)), (2 ** 30, 2 ** 30, (2, 2, 0))]
GOOD = [(20, 36, (12, 16, 2)), (20, 36, (12, 16, 5)), (20, 36, (0, 0, 0)), (20, 36, (0, 0, 99)), (20, 36, (40, 16, 7)), (20, 36, (20, 36, 30)),
        (34, 66, (14, 32, 4, 3))]


def test_check_refuses():
    for H, W, t in BAD:
        with pytest.raises(ValueError, match="tile"):
            tiles.check(H, W, t)
    for H, W, t in GOOD:
        assert tiles.check(H, W, t) == tiles.tiling(t)
    for t in (None, 8, (8,), (8, 8, 0, 0, 0), (8.0, 8), ("8", "8"), (True, 8), "88"):
        with pytest.raises(ValueError):
            tiles.tiling(t)
    for args in ((35, 16, 2), (36, 15, 2), (36, 16, -1), (36, 16, 8), (0, 16, 2)):
        with pytest.raises(ValueError):
            tiles.axis(*args)


def test_capi_axis_equals_the_rule():
    lib = _capi.load_library()
    assert lib.pfnl_version() == 4
    for n, t, p in _legal():
        want = tiles.axis(n, t, p)
        count = C.c_int(-1)
        assert lib.pfnl_tile_axis(n, t, p, C.byref(count), None, None, None) == 0 and count.value == len(want)   # NULL arrays: the count only
        o, a, c = ((C.c_int32 * (count.value + 1))(*([-7] * (count.value + 1))) for _ in range(3))
        assert lib.pfnl_tile_axis(n, t, p, C.byref(count), o, a, c) == 0
        assert [(o[i], a[i], a[i] + c[i]) for i in range(count.value)] == want, (n, t, p)
        assert o[count.value] == a[count.value] == c[count.value] == -7          # nothing past the count
    count = C.c_int(0)
    for args, word in (((35, 16, 2), b" n "), ((0, 16, 2), b" n "), ((-4, 16, 2), b" n "), ((36, 15, 2), b"tile extent"), ((36, -2, 0), b"tile extent"),
                       ((36, 16, -1), b"pad"), ((36, 16, 8), b"pad"), ((36, 16, 2 ** 31 - 1), b"pad")):
        assert lib.pfnl_tile_axis(*args, C.byref(count), None, None, None) == -1, args
        assert word in lib.pfnl_last_error(), (args, lib.pfnl_last_error())
    assert lib.pfnl_tile_axis(36, 16, 2, None, None, None, None) == -1 and b"NULL" in lib.pfnl_last_error()


@pytest.mark.parametrize("B,H,W,tile", [(1, 20, 36, (12, 16, 2)), (3, 34, 66, (14, 32, 3)), (2, 34, 26, (14, 0, 3)), (2, 12, 20, (8, 12, 1)),
                                        (1, 6, 10, (0, 0, 0)), (2, 16, 16, (6, 6, 2))])
def test_assemble_of_split_with_a_pointwise_forward_is_exact(B, H, W, tile):
    """nearest-neighbour x scale of the centre frame commutes with cropping: the tiled result IS f of the whole frame"""
    T = 3
    x = np.random.default_rng(H * W + B).random((B, T, H, W, 3), dtype=np.float32)
    for scale in (4, 2):
        f = lambda a: np.repeat(np.repeat(a[:, T // 2], scale, axis=-3), scale, axis=-2)[:, None]   # noqa: E731
        want = f(x)
        for batch in (0, 1, 3):
            t = tile + (batch,)
            got = tiles.forward_tiled(f, x, t)
            assert got.dtype == np.float32 and got.shape == (B, 1, scale * H, scale * W, 3) and np.array_equal(got, want), (scale, batch)
        stack = tiles.split(x, tile)
        th, tw, rows, cols = tiles.grid(H, W, tile)
        assert stack.flags["C_CONTIGUOUS"] and stack.shape == (B * len(rows) * len(cols), T, th, tw, 3)
        assert np.array_equal(tiles.assemble(f(stack), B, H, W, scale, tile), want)            # one array of all results
        assert np.array_equal(tiles.assemble(f(stack)[:, 0], B, H, W, scale, tile), want[:, 0])  # ... without the frame axis
        # the numbering: clip-major, then the row of tiles, then the column
        k = (B - 1) * len(rows) * len(cols) + (len(rows) - 1) * len(cols)
        oy, ox = rows[-1][0], cols[0][0]
        assert np.array_equal(stack[k], x[B - 1, :, oy:oy + th, ox:ox + tw])
    if tile == (14, 32, 3):
        assert any((b - a) % 2 for _, a, b in tiles.axis(W, 32, 3)) and any((b - a) % 2 for _, a, b in tiles.axis(H, 14, 3))   # odd owned widths
    with pytest.raises(ValueError):
        tiles.assemble(f(stack)[1:], B, H, W, 2, tile)


def test_the_margin_is_what_makes_the_trunk_exact():
    """With the non-local block's output projection zeroed the block is the identity and the network is its convolutions, whose
    receptive field is 4 + 2 num_block = 6 LR pixels: tiles with pad 6 reproduce the whole frame within the forward bound, pad 0 does not."""
    from oracle import pfnl_fast
    geom = PFNLGeometry(num_block=1)
    w = dict(synth.synthetic_weights(geom, seed=0))
    for leaf in ("kernel", "bias"):
        w[f"nlvsr/nlblock_0/w/w/{leaf}"] = np.zeros_like(w[f"nlvsr/nlblock_0/w/w/{leaf}"])
    fo = pfnl_fast.FastOracle(w, num_block=1)
    f = lambda a: fo.forward(np.ascontiguousarray(a))                            # noqa: E731
    x = synth.uniform_clips(1, 7, 24, 40, seed=31)
    whole = f(x)
    assert whole.shape == (1, 1, 96, 160, 3)
    assert len(tiles.axis(24, 16, 6)) == 3 and len(tiles.axis(40, 16, 6)) == 7
    padded = tiles.forward_tiled(f, x, (16, 16, 6))
    err = float(np.abs(padded - whole).max())
    bare = float(np.abs(tiles.forward_tiled(f, x, (16, 16, 0)) - whole).max())
    print(f"\n[tiles] oracle, projection zeroed: max |tiled - whole| pad 6: {err:.3g}, pad 0: {bare:.3g}", end="")
    assert err < ABS_TOL, err
    assert not bare < ABS_TOL, bare


# ---- tile_geom.h, stand-alone --------------------------------------------------------------------------------------------------------
DRIVER = r"""
#include <cstdio>
#include "tile_geom.h"
int main() {
    int H, W;
    pfnl_tiling t;
    while (std::scanf("%d %d %d %d %d %d", &H, &W, &t.tile_h, &t.tile_w, &t.pad, &t.batch) == 6) {
        const char* why = pfnl::tiling_refused(H, W, t);
        if (why) {
            std::printf("X %s\n", why);
            continue;
        }
        const pfnl::TileGrid g = pfnl::tile_grid(H, W, t);
        const int total = pfnl::tile_total(g, 2);
        std::printf("G %d %d %d %d %d %d |", g.y.extent, g.x.extent, g.y.count, g.x.count, total, total ? pfnl::tile_run(total, t.batch) : 0);
        const int show = total < 64 ? total : 64;
        for (int k = 0; k < show; ++k) {
            const pfnl::TilePos p = pfnl::tile_pos(g, k);
            std::printf(" %d %d %d %d %d %d %d", p.b, p.oy, p.ox, p.ay, p.by, p.ax, p.bx);
        }
        std::printf("\n");
    }
    return 0;
}
"""
CASES = BAD + GOOD + [(H, W, (th, tw, p, b)) for H, W in ((12, 20), (34, 26)) for th in (0, 6, 8, 14) for tw in (0, 4, 12, 26)
                      for p in (0, 1, 2, 3) for b in (0, 5)]


def _compiler():
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++") if c and os.path.exists(c)), None)
    assert cxx, "no host C++ compiler (the build's own clang++ is the last candidate)"
    return cxx


def _build_and_run(tmp_path, name, extra=()):
    src, exe = tmp_path / "driver.cpp", tmp_path / name
    src.write_text(DRIVER)
    subprocess.run([_compiler(), "-std=c++17", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "pfnl_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    lines = "".join("%d %d %d %d %d %d\n" % ((H, W) + tiles_4(t)) for H, W, t in CASES)
    return subprocess.run([str(exe)], input=lines, check=True, capture_output=True, text=True).stdout


def tiles_4(t):
    return tuple(t) + (0, 0)[:4 - len(t)]                                        # (the refused entries included, as they stand)


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return _build_and_run(tmp_path_factory.mktemp("tiles"), "driver")


def test_tile_geom_header_equals_the_rule(table):
    lines = table.strip().split("\n")
    assert len(lines) == len(CASES)
    refused = 0
    for (H, W, t), line in zip(CASES, lines):
        try:
            tiles.check(H, W, t)
        except ValueError:
            assert line.startswith("X tile"), (H, W, t, line)
            refused += 1
            continue
        assert line.startswith("G "), (H, W, t, line)
        head, _, body = line[2:].partition("|")
        th, tw, rows, cols = tiles.grid(H, W, t)
        total = 2 * len(rows) * len(cols)
        batch = tiles_4(t)[3]
        assert [int(v) for v in head.split()] == [th, tw, len(rows), len(cols), total, tiles.runs(total, batch)[0][1]], (H, W, t)
        want = [(b, oy, ox, ay, by, ax, bx) for b in range(2) for oy, ay, by in rows for ox, ax, bx in cols][:64]
        got = [int(v) for v in body.split()]
        assert [tuple(got[i:i + 7]) for i in range(0, len(got), 7)] == want, (H, W, t)
    assert refused == len(BAD) + sum(1 for H, W, t in CASES[len(BAD) + len(GOOD):] if _refuses(H, W, t)) and refused > len(BAD)


def _refuses(H, W, t):
    try:
        tiles.check(H, W, t)
    except ValueError:
        return True
    return False


def test_the_driver_is_clean_under_the_sanitizers(table, tmp_path):
    """a stand-alone program: the sanitizers' runtimes are linked into it, nothing is preloaded"""
    assert _build_and_run(tmp_path, "driver_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")) == table


# ---- refusals without a device -------------------------------------------------------------------------------------------------------
def test_capi_refuses_without_a_device():
    lib = _capi.load_library()
    dummy = C.c_void_p(16)                                                       # never dereferenced: the calls return first
    ok = _capi.pfnl_tiling(12, 16, 2, 0)
    fwd = lambda h, t, n=1, H=20, W=36: lib.pfnl_forward_tiled(h, dummy, 1, dummy, 1, 1, H, W, t, n, None)   # noqa: E731
    assert fwd(dummy, C.byref(ok), 3) == -1 and b"ensemble" in lib.pfnl_last_error()
    assert fwd(None, C.byref(ok)) == -1 and b"NULL" in lib.pfnl_last_error()
    assert fwd(None, None) == -1 and b"NULL" in lib.pfnl_last_error()            # no tiling: pfnl_forward_ensemble's own checks
    assert fwd(dummy, C.byref(ok), H=21) == -1 and b"even" in lib.pfnl_last_error()
    assert fwd(dummy, C.byref(ok), W=0) == -1 and b"positive" in lib.pfnl_last_error()
    for H, W, t in BAD[3:-1]:
        assert fwd(dummy, C.byref(_capi.pfnl_tiling(*tiles_4(t))), H=H, W=W) == -1 and b"tile" in lib.pfnl_last_error(), t
    assert lib.pfnl_forward_tiled(dummy, dummy, 1, dummy, 1, 2 ** 20, 2 ** 12, 2 ** 12, C.byref(_capi.pfnl_tiling(2, 2, 0, 0)), 1, None) == -1
    assert b"overflows" in lib.pfnl_last_error()                                 # 2^20 clips of 2^22 tiles
    for fn, args in ((lib.pfnl_op_tile_gather, (1, 7, 20, 36)), (lib.pfnl_op_tile_scatter, (1, 20, 36, 4))):
        assert fn(None, dummy, *args, C.byref(ok), 0, 1, None) == -1 and b"NULL" in lib.pfnl_last_error()
        assert fn(dummy, None, *args, C.byref(ok), 0, 1, None) == -1 and b"NULL" in lib.pfnl_last_error()
        assert fn(dummy, dummy, *args, None, 0, 1, None) == -1 and b"NULL" in lib.pfnl_last_error()
        assert fn(dummy, dummy, *args, C.byref(_capi.pfnl_tiling(12, 16, 6, 0)), 0, 1, None) == -1 and b"pad" in lib.pfnl_last_error()
        for first, count in ((-1, 1), (0, 0), (0, 7), (5, 2), (6, 1)):           # 2 x 3 tiles
            assert fn(dummy, dummy, *args, C.byref(ok), first, count, None) == -1 and b"tiles of the call" in lib.pfnl_last_error()
    assert lib.pfnl_op_tile_gather(dummy, dummy, 0, 7, 20, 36, C.byref(ok), 0, 1, None) == -1 and b" B " in lib.pfnl_last_error()
    assert lib.pfnl_op_tile_gather(dummy, dummy, 1, 0, 20, 36, C.byref(ok), 0, 1, None) == -1 and b" T " in lib.pfnl_last_error()
    assert lib.pfnl_op_tile_scatter(dummy, dummy, 1, 20, 36, 0, C.byref(ok), 0, 1, None) == -1 and b"scale" in lib.pfnl_last_error()
    assert lib.pfnl_stream_tile(None, C.byref(ok)) == -1 and b"NULL" in lib.pfnl_last_error()
    assert lib.pfnl_stream_tile(None, None) == -1 and b"NULL" in lib.pfnl_last_error()


def test_tile_arguments_are_checked_before_anything_touches_the_engine():
    from pfnl_amd.engine import PFNLEngine, tile_argument
    from pfnl_amd.model import PFNL
    from pfnl_amd.stream import VideoStream, tiling_argument
    assert inspect.signature(PFNLEngine.forward).parameters["tile"].default is None
    assert inspect.signature(PFNLEngine.forward_device).parameters["tile"].default is None
    assert PFNL().tile is None and PFNL.tile is None
    assert list(inspect.signature(VideoStream.set_tiling).parameters) == ["self", "tile_h", "tile_w", "pad", "batch"]
    assert isinstance(VideoStream.tiling, property)
    assert tile_argument(None, (1, 7, 20, 36, 3)) is None
    t = tile_argument((12, 16, 2), (1, 7, 20, 36, 3))
    assert isinstance(t, _capi.pfnl_tiling) and (t.tile_h, t.tile_w, t.pad, t.batch) == (12, 16, 2, 0)
    assert tiling_argument(20, 36, 12, 16) == (12, 16, 0, 0) and tiling_argument(20, 36, 12, 16, 2, 5) == (12, 16, 2, 5)

    class Unready:                                                               # no handle, no library, no weights
        ensemble, tile, H, W = 1, None, 20, 36
    x = np.zeros((1, 7, 20, 36, 3), np.float32)
    for bad in ((11, 16), (12, 16, 6), (12, 16, -1), (12, 16, 2, -1), (12,), "12", (12.0, 16)):
        with pytest.raises(ValueError, match="tile"):
            PFNLEngine.forward(Unready(), x, tile=bad)
        with pytest.raises(ValueError, match="tile"):
            PFNLEngine.forward_device(Unready(), 16, 16, 1, 20, 36, tile=bad)
        with pytest.raises(ValueError, match="tile"):
            tile_argument(bad, x.shape)
    for bad in ((11, 16), (12, 16, 6), (12, 16, -1), (12, 16, 2, -1), (12.0, 16)):
        with pytest.raises(ValueError, match="tile"):
            VideoStream.set_tiling(Unready(), *bad)
        with pytest.raises(ValueError, match="tile"):
            tiling_argument(20, 36, *bad)
    bad_default = Unready()
    bad_default.tile = (11, 16)                                                  # the engine's own default goes through the same check
    with pytest.raises(ValueError, match="tile"):
        PFNLEngine.forward(bad_default, x)
