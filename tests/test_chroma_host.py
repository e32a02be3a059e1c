"""4:2:2 and 4:4:4 without a device (include/pfnl_hip.h CHROMA FORMAT): the rule of pfnl_amd/yuv.py / pfnl_amd/depth10.py with chroma = "422" |
"444" - known answers, its two ties to the 4:2:0 rule, the positions in exact rationals, the standards' equations -, the layouts, the C-ABI's
refusals, the host-only headers as a plain C++ program (once more under the sanitizers), Y4M's four tags and the upscale loop around a stub."""
import ctypes as C
import io
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from conftest import ROOT
from pfnl_amd import _capi, depth10, surface, y4m, yuv
from pfnl_amd import upscale as up
from pfnl_amd.stream import (chroma_arguments, frame_dtype, frame_shapes, output_grid, placement_arguments, resize_arguments)
from test_route_host import _compiler
from test_siting_host import _bilinear_taps, _footprint_taps, _round_half_up
from test_yuv_host import _real_constants

NEW = ("422", "444")
PAIRS = [("bt601", False), ("bt601", True), ("bt709", False), ("bt709", True)]
HOOKS = ("pfnl_op_yuv_to_rgb_u8_chroma", "pfnl_op_yuv_to_rgb_u10_chroma", "pfnl_op_yuv_to_rgb_u8_surface_chroma",
         "pfnl_op_yuv_to_rgb_u10_surface_chroma", "pfnl_op_rgb_to_yuv_u8_chroma", "pfnl_op_rgb_to_yuv_u10_chroma")


# ---- 1. known answers ---------------------------------------------------------------------------------------------------------------------
def test_the_names_are_the_abi_values():
    assert yuv.CHROMAS == ("420", "422", "444") and [yuv.chroma_id(c) for c in yuv.CHROMAS] == [0, 1, 2]
    assert _capi.CHROMA_FORMATS == {c: k for k, c in enumerate(yuv.CHROMAS)}
    for bad in ("4:2:2", 422, None, "411"):
        with pytest.raises(ValueError):
            yuv.chroma_id(bad)


@pytest.mark.parametrize("chroma", NEW)
def test_greys_white_and_black(chroma):
    H, W = 3, 4
    rng = np.random.default_rng(1)
    grey = np.repeat(rng.integers(0, 256, (H, W, 1), dtype=np.uint8), 3, axis=2)
    grey10 = np.repeat(rng.integers(0, 1024, (H, W, 1)).astype(np.uint16), 3, axis=2)
    for matrix, full in PAIRS:
        for fmt, fmt10 in (("nv12", "p010"), ("i420", "i010")):
            for siting in yuv.SITINGS:
                _, cb, cr = yuv.planes(yuv.from_rgb(grey, fmt, matrix, full, siting=siting, chroma=chroma), fmt, H, W, chroma)
                assert (cb == 128).all() and (cr == 128).all()
                _, cb, cr = depth10.planes10(depth10.from_rgb10(grey10, fmt10, matrix, full, siting=siting, chroma=chroma), fmt10, H, W, chroma)
                assert (cb == 512).all() and (cr == 512).all()
            for level, y8, y10 in ((255, 255 if full else 235, 1023 if full else 940), (0, 0 if full else 16, 0 if full else 64)):
                y, cb, cr = yuv.planes(yuv.from_rgb(np.full((H, W, 3), level, np.uint8), fmt, matrix, full, chroma=chroma), fmt, H, W, chroma)
                assert (y == y8).all() and (cb == 128).all() and (cr == 128).all()
                frame = yuv.pack(y, cb, cr, fmt, chroma)
                assert (yuv.to_rgb(frame, fmt, H, W, matrix, full, chroma=chroma) == level).all()          # and back, exactly
                level10 = 1023 if level else 0
                f10 = depth10.from_rgb10(np.full((H, W, 3), level10, np.uint16), fmt10, matrix, full, chroma=chroma)
                y, cb, cr = depth10.planes10(f10, fmt10, H, W, chroma)
                assert (y == y10).all() and (cb == 512).all() and (cr == 512).all()
                assert (depth10.to_rgb10(f10, fmt10, H, W, matrix, full, chroma=chroma) == level10).all()


def test_one_row_of_four_by_hand():
    """4:2:2, chroma samples (10, 201) under four luma pixels.  Co-sited: pixel 0 and 2 sit on their samples, pixel 1 is (2 * 10 + 2 * 201 + 2)
    >> 2 = 106, pixel 3's far sample clamps onto 201.  Midway: (3 near + far + 2) >> 2 with the far index clamped at both ends:
    (30 + 10 + 2) >> 2 = 10, (30 + 201 + 2) >> 2 = 58, (603 + 10 + 2) >> 2 = 153, (603 + 201 + 2) >> 2 = 201.
    Encode, numerators (10, -20, 40, -7) << 14.  Co-sited, column -1 clamped onto 0: (3 * 10 - 20) / 4 = 2.5 -> 3, (-20 + 80 - 7) / 4 = 13.25
    -> 13.  Midway: (10 - 20) / 2 = -5, (40 - 7) / 2 = 16.5 -> 17."""
    c = np.array([[10, 201]])
    for siting in ("left", "topleft"):
        assert yuv.upsample(c, 1, 4, siting, "422").tolist() == [[10, 106, 201, 201]]
    assert yuv.upsample(c, 1, 4, "center", "422").tolist() == [[10, 58, 153, 201]]
    assert yuv.upsample(np.array([[10, 106, 201, 7]]), 1, 4, "center", "444").tolist() == [[10, 106, 201, 7]]
    num = np.array([[10, -20, 40, -7]]) << yuv.F
    for siting in ("left", "topleft"):
        assert yuv.encode_filter(num, siting, "422")[1] == 2
        assert yuv.downsample(num, siting, "422").tolist() == [[131, 141]]
        assert depth10.downsample10(num, siting, "422").tolist() == [[515, 525]]
    assert yuv.encode_filter(num, "center", "422")[1] == 1
    assert yuv.downsample(num, "center", "422").tolist() == [[123, 145]]
    assert depth10.downsample10(num, "center", "422").tolist() == [[507, 529]]
    s, k = yuv.encode_filter(num + 5000, "left", "444")
    assert k == 0 and np.array_equal(s, num + 5000)
    assert yuv.downsample(num + 8191, "center", "444").tolist() == [[138, 108, 168, 121]]        # (N + HALF) >> F: just below a half stays
    assert yuv.downsample(num + 8192, "center", "444").tolist() == [[139, 109, 169, 122]]        # and a half goes up


# ---- 2. the ties to the 4:2:0 rule ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("siting", yuv.SITINGS)
@pytest.mark.parametrize("H,W", [(2, 2), (4, 2), (6, 10), (2, 36)])
def test_equal_rows_make_422_the_420_rule(H, W, siting):
    rng = np.random.default_rng(H * 100 + W)
    for top in (256, 1024):
        row = rng.integers(0, top, (1, W // 2))
        assert np.array_equal(yuv.upsample(np.repeat(row, H // 2, 0), H, W, siting, chroma="420"), yuv.upsample(np.repeat(row, H, 0), H, W, siting, "422"))
    rgb = np.repeat(rng.integers(0, 256, (1, W, 3), dtype=np.uint8), H, 0)
    rgb10 = np.repeat(rng.integers(0, 1024, (1, W, 3)).astype(np.uint16), H, 0)
    for matrix, full in PAIRS[::3]:
        a = yuv.planes(yuv.from_rgb(rgb, "i420", matrix, full, siting=siting), "i420", H, W)
        b = yuv.planes(yuv.from_rgb(rgb, "i420", matrix, full, siting=siting, chroma="422"), "i420", H, W, "422")
        assert np.array_equal(a[0], b[0]) and all((b[k] == a[k][0]).all() for k in (1, 2))
        a = depth10.planes10(depth10.from_rgb10(rgb10, "i010", matrix, full, siting=siting), "i010", H, W)
        b = depth10.planes10(depth10.from_rgb10(rgb10, "i010", matrix, full, siting=siting, chroma="422"), "i010", H, W, "422")
        assert np.array_equal(a[0], b[0]) and all((b[k] == a[k][0]).all() for k in (1, 2))


def test_what_of_a_siting_each_subsampling_reads():
    rng = np.random.default_rng(5)
    H, W = 3, 6
    rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    f422 = {s: yuv.from_rgb(rgb, "nv12", siting=s, chroma="422") for s in yuv.SITINGS}
    assert np.array_equal(f422["left"], f422["topleft"]) and not np.array_equal(f422["left"], f422["center"])
    d422 = {s: yuv.to_rgb(f422["left"], "nv12", H, W, siting=s, chroma="422") for s in yuv.SITINGS}
    assert np.array_equal(d422["left"], d422["topleft"]) and not np.array_equal(d422["left"], d422["center"])
    f444 = [yuv.from_rgb(rgb, "i420", siting=s, chroma="444") for s in yuv.SITINGS]
    assert all(np.array_equal(f, f444[0]) for f in f444)
    d444 = [yuv.to_rgb(f444[0], "i420", H, W, siting=s, chroma="444") for s in yuv.SITINGS]
    assert all(np.array_equal(d, d444[0]) for d in d444)
    rgb10 = rng.integers(0, 1024, (H, W, 3)).astype(np.uint16)
    assert np.array_equal(depth10.from_rgb10(rgb10, "p010", siting="left", chroma="422"), depth10.from_rgb10(rgb10, "p010", siting="topleft", chroma="422"))
    assert np.array_equal(depth10.from_rgb10(rgb10, "i010", siting="left", chroma="444"), depth10.from_rgb10(rgb10, "i010", siting="center", chroma="444"))


# ---- 3. the positions, in exact rationals: one axis of tests/test_siting_host.py ---------------------------------------------------------------
@pytest.mark.parametrize("siting", yuv.SITINGS)
@pytest.mark.parametrize("H,W", [(1, 2), (3, 6), (2, 10)])
def test_422_is_the_horizontal_filter_at_the_positions(H, W, siting):
    rng = np.random.default_rng(H * 31 + W)
    ox = Fraction(1, 2) if yuv.AXES[siting][1] else Fraction(0)
    c = rng.integers(0, 256, (H, W // 2))
    got = yuv.upsample(c, H, W, siting, "422")
    num = rng.integers(-128 << yuv.F, 128 << yuv.F, (H, W)).astype(np.int32)
    s, k = yuv.encode_filter(num, siting, "422")
    assert k == (1 if ox else 2) and s.shape == (H, W // 2)
    down, down10 = yuv.downsample(num, siting, "422"), depth10.downsample10(num.astype(np.int64) * 4, siting, "422")
    for y in range(H):
        for x in range(W):
            assert got[y, x] == _round_half_up(sum(wx * int(c[y, i]) for i, wx in _bilinear_taps(x, ox, W // 2))), (siting, y, x)
        for i in range(W // 2):
            v = sum(wx * int(num[y, x]) for x, wx in _footprint_taps(i, ox, W))
            assert Fraction(int(s[y, i]), 1 << k) == v, (siting, y, i)
            assert down[y, i] == min(max(128 + _round_half_up(v / (1 << yuv.F)), 0), 255)
            assert down10[y, i] == min(max(512 + _round_half_up(4 * v / (1 << yuv.F)), 0), 1023)


# ---- 4. the standards' equations at 4:4:4 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matrix,full", PAIRS)
def test_444_both_ways_is_within_one_code_of_the_real_formula(matrix, full):
    """A grid of colours, one pixel each - at 4:4:4 a pixel is a flat colour.  The bound is the one tests/test_yuv_host.py holds the 4:2:0 rule
    to on flat colour, for the reason given there: the integer numerator is within 0.04 code of the real one ahead of the one rounding, so
    the two roundings differ by at most 1 - on the way out, and on the way back from the samples the way out gave."""
    kr, kg, kb, y0, ys, cs = _real_constants(matrix, full)
    half_up = lambda x: np.clip(np.floor(x + 0.5), 0, 255).astype(np.int32)      # noqa: E731
    v = np.arange(0, 256, 5)
    colours = np.stack(np.meshgrid(v, v, v, indexing="ij"), axis=-1).reshape(1, -1, 3).astype(np.uint8)
    n = colours.shape[1]
    frame = yuv.from_rgb(colours, "i420", matrix, full, chroma="444")
    Y, Cb, Cr = (p.astype(np.float64)[0] for p in yuv.planes(frame, "i420", 1, n, "444"))
    R, G, B = (colours[0, :, k].astype(np.float64) for k in range(3))
    yf = kr * R + kg * G + kb * B
    want = (half_up(y0 + ys * yf), half_up(128.0 + cs * (B - yf) / (2.0 * (1.0 - kb))), half_up(128.0 + cs * (R - yf) / (2.0 * (1.0 - kr))))
    assert max(int(np.abs(g - w).max()) for g, w in zip((Y, Cb, Cr), want)) <= 1
    back = yuv.to_rgb(frame, "i420", 1, n, matrix, full, chroma="444")[0].astype(np.int32)
    yn, U, V = (Y - y0) / ys, (Cb - 128.0) / cs, (Cr - 128.0) / cs
    real = np.stack([half_up(yn + 2.0 * (1.0 - kr) * V), half_up(yn - 2.0 * kb * (1.0 - kb) / kg * U - 2.0 * kr * (1.0 - kr) / kg * V),
                     half_up(yn + 2.0 * (1.0 - kb) * U)], axis=-1)
    assert int(np.abs(back - real).max()) <= 1


# ---- 5. layouts -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chroma,H,W", [("422", 1, 2), ("422", 3, 6), ("444", 1, 1), ("444", 3, 5)])
def test_layouts_sizes_and_round_trips(chroma, H, W):
    rng = np.random.default_rng(H * 10 + W)
    ch, cw = yuv.chroma_shape(H, W, chroma)
    assert (ch, cw) == (H, W // 2 if chroma == "422" else W)
    assert yuv.frame_bytes(H, W, chroma) == depth10.frame_samples(H, W, chroma) == (2 if chroma == "422" else 3) * H * W
    Y, Cb, Cr = rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (ch, cw), dtype=np.uint8), rng.integers(0, 256, (ch, cw), dtype=np.uint8)
    for fmt in yuv.FORMATS:
        frame = yuv.pack(Y, Cb, Cr, fmt, chroma)
        assert frame.shape == (yuv.frame_bytes(H, W, chroma) // W, W) and frame.dtype == np.uint8
        assert all(np.array_equal(a, b) for a, b in zip(yuv.planes(frame, fmt, H, W, chroma), (Y, Cb, Cr)))
        assert all(np.array_equal(a, b) for a, b in zip(yuv.planes(frame.reshape(-1), fmt, H, W, chroma), (Y, Cb, Cr)))
        flat = frame.reshape(-1)
        assert np.array_equal(flat[:H * W].reshape(H, W), Y)
        if fmt == "nv12":
            assert np.array_equal(flat[H * W:].reshape(ch, cw, 2)[..., 1], Cr)
        else:
            assert np.array_equal(flat[H * W + ch * cw:].reshape(ch, cw), Cr)
        with pytest.raises(ValueError):
            yuv.planes(flat[:-1], fmt, H, W, chroma)
        with pytest.raises(ValueError):
            yuv.pack(Y, Cb[:, :-1] if cw > 1 else Cb[:0], Cr, fmt, chroma)
    Y10, Cb10, Cr10 = (p.astype(np.uint16) * 4 + 3 for p in (Y, Cb, Cr))
    for fmt in depth10.FORMATS:
        frame = depth10.pack10(Y10, Cb10, Cr10, fmt, chroma)
        assert frame.shape == (depth10.frame_samples(H, W, chroma) // W, W) and frame.dtype == np.uint16
        assert all(np.array_equal(a, b) for a, b in zip(depth10.planes10(frame, fmt, H, W, chroma), (Y10, Cb10, Cr10)))
        assert int(frame.max()) <= (1023 << depth10.SHIFT[fmt])
    p210 = depth10.pack10(Y10, Cb10, Cr10, "p010", chroma)
    assert np.array_equal(depth10.values10(p210 | 63, "p010", chroma), p210 >> 6)                # the low six bits are ignored
    assert depth10.values10(np.array([1023, 1024, 65535], np.uint16), "i010", chroma).tolist() == [1023, 1023, 1023]
    with pytest.raises(ValueError):
        depth10.values10(p210, "p010", "440")


def test_sizes_each_subsampling_takes():
    for chroma, good, bad in (("420", [(2, 2)], [(1, 2), (2, 3), (3, 2)]), ("422", [(1, 2), (3, 6)], [(2, 3), (1, 1), (0, 2)]),
                              ("444", [(1, 1), (3, 5)], [(0, 1), (1, 0)])):
        for H, W in good:
            yuv.check_size(H, W, chroma)
        for H, W in bad:
            with pytest.raises(ValueError):
                yuv.check_size(H, W, chroma)
            with pytest.raises(ValueError):
                yuv.from_rgb(np.zeros((H, W, 3), np.uint8), "nv12", chroma=chroma)
    assert yuv.frame_bytes(4, 6) == 36 and depth10.frame_samples(4, 6) == 36                      # the calls without the keyword


# ---- 6. the C-ABI without a device ---------------------------------------------------------------------------------------------------------------
def test_chroma_entries_are_declared_and_refuse_without_a_device():
    assert set(HOOKS) | {"pfnl_stream_chroma_format"} <= set(_capi.SIGNATURES)
    lib = _capi.load_library()
    assert lib.pfnl_version() == 4                                       # symbols were added, nothing changed
    dummy, odd = C.c_void_p(16), C.c_void_p(17)                          # never dereferenced: the calls return first
    sf = _capi.pfnl_surface()
    for k in range(3):
        sf.plane[k], sf.pitch[k] = 4096, 64
    err = lib.pfnl_last_error
    packed = [(lib.pfnl_op_yuv_to_rgb_u8_chroma, 1, 2), (lib.pfnl_op_rgb_to_yuv_u8_chroma, 2, 1),
              (lib.pfnl_op_yuv_to_rgb_u10_chroma, 4, 5), (lib.pfnl_op_rgb_to_yuv_u10_chroma, 5, 4)]
    for op, fmt, other in packed:
        call = lambda a=dummy, f=fmt, m=1, fr=0, n=1, H=3, W=6, b=dummy, c=1, s=0: op(a, f, m, fr, n, H, W, b, c, s, None)   # noqa: E731
        for chroma in (1, 2):
            assert call(a=None, c=chroma) == -1 and b"NULL" in err()
            assert call(b=None, c=chroma) == -1 and b"NULL" in err()
            assert call(f=0, c=chroma) == -1 and b"fmt" in err()                                   # an RGB fmt
            assert call(f=3, c=chroma) == -1 and b"fmt" in err()
            assert call(f=6, c=chroma) == -1 and b"fmt" in err()
            assert call(f=(4 if fmt < 3 else 1), c=chroma) == -1 and b"fmt" in err()               # the other depth's layout
            assert call(m=2, c=chroma) == -1 and b"matrix" in err()
            assert call(fr=2, c=chroma) == -1 and b"full_range" in err()
            assert call(n=0, c=chroma) == -1 and b"n >= 1" in err()
            assert call(H=0, c=chroma) == -1 and call(W=0, c=chroma) == -1 and call(W=-2, c=chroma) == -1
            for bad in (-1, 3):
                assert call(s=bad, c=chroma) == -1 and b"siting" in err()
            if fmt > 3:
                assert call(a=odd, c=chroma) == -1 and b"2-byte aligned" in err()
                assert call(b=odd, c=chroma) == -1 and b"2-byte aligned" in err()
        assert call(W=5, c=1) == -1 and b"even" in err() and b"4:2:2" in err()
        for bad in (-1, 3, 7):
            assert call(c=bad) == -1 and b"chroma" in err()
        assert call(f=other, a=None) == -1                                                         # (the other layout of the depth is one)
    for op, fmt in ((lib.pfnl_op_yuv_to_rgb_u8_surface_chroma, 2), (lib.pfnl_op_yuv_to_rgb_u10_surface_chroma, 5)):
        call = lambda a=C.byref(sf), f=fmt, m=1, fr=0, H=4, W=6, b=dummy, c=1, s=0: op(a, f, m, fr, H, W, b, c, s, None)   # noqa: E731
        for chroma in (1, 2):
            assert call(a=None, c=chroma) == -1 and b"NULL" in err()
            assert call(b=None, c=chroma) == -1 and b"NULL" in err()
            assert call(f=0, c=chroma) == -1 and b"fmt" in err()
            assert call(m=-1, c=chroma) == -1 and b"matrix" in err()
            assert call(s=3, c=chroma) == -1 and b"siting" in err()
            assert call(W=128, c=chroma) == -1 and b"pitch" in err()                               # a row of 128 samples under a pitch of 64
        if fmt == 5:
            assert call(W=64, c=1, f=4) == -1 and b"pitch" in err()                                # P210: 64 samples are 128 bytes
        assert call(W=40, c=2, f=fmt - 1) == -1 and b"pitch" in err()                              # NV24 / P410: CbCr rows of 2 W samples
        assert call(W=5, c=1) == -1 and b"even" in err()
        assert call(c=3) == -1 and b"chroma" in err()
        sf.plane[1] = None
        assert call(c=2) == -1 and b"plane" in err()
        sf.plane[1] = 4096
        if fmt == 5:
            sf.pitch[2] = 65
            assert call(c=2) == -1 and b"even" in err()
            sf.pitch[2] = 64
            assert call(b=odd) == -1 and b"2-byte aligned" in err()
    for bad in (-1, 3):
        assert lib.pfnl_stream_chroma_format(dummy, bad, 0) == -1 and b"chroma format" in err()
        assert lib.pfnl_stream_chroma_format(dummy, 0, bad) == -1 and b"chroma format" in err()
    assert lib.pfnl_stream_chroma_format(None, 1, 1) == -1 and b"NULL" in err()


def test_chroma_420_is_forwarded_to_the_sited_hooks():
    """the same refusals, in the same words, as the _sited twins give"""
    lib = _capi.load_library()
    dummy = C.c_void_p(16)
    sf = _capi.pfnl_surface()
    for k in range(3):
        sf.plane[k], sf.pitch[k] = 4096, 64
    pairs = [(lib.pfnl_op_yuv_to_rgb_u8_chroma, lib.pfnl_op_yuv420_to_rgb_u8_sited, 1), (lib.pfnl_op_rgb_to_yuv_u8_chroma, lib.pfnl_op_rgb_to_yuv420_u8_sited, 2),
             (lib.pfnl_op_yuv_to_rgb_u10_chroma, lib.pfnl_op_yuv420_to_rgb_u10_sited, 4), (lib.pfnl_op_rgb_to_yuv_u10_chroma, lib.pfnl_op_rgb_to_yuv420_u10_sited, 5)]
    cases = [dict(a=None), dict(b=None), dict(f=0), dict(m=2), dict(fr=-1), dict(n=0), dict(H=3), dict(W=5), dict(H=0), dict(s=3), dict(a=C.c_void_p(17))]
    for new, old, fmt in pairs:
        for case in cases:
            kw = dict(a=dummy, f=fmt, m=1, fr=0, n=1, H=4, W=6, b=dummy, s=0)
            kw.update(case)
            head = (kw["a"], kw["f"], kw["m"], kw["fr"], kw["n"], kw["H"], kw["W"], kw["b"])
            if "a" in case and case["a"] is not None and fmt < 3:
                continue                                                                           # (an odd pointer is fine for bytes: it would launch)
            r_old = old(*head, kw["s"], None)
            text_old = lib.pfnl_last_error()
            assert new(*head, 0, kw["s"], None) == r_old == -1 and lib.pfnl_last_error() == text_old, (fmt, case)
    for new, old, fmt in ((lib.pfnl_op_yuv_to_rgb_u8_surface_chroma, lib.pfnl_op_yuv420_to_rgb_u8_surface_sited, 1),
                          (lib.pfnl_op_yuv_to_rgb_u10_surface_chroma, lib.pfnl_op_yuv420_to_rgb_u10_surface_sited, 4)):
        for case in (dict(a=None), dict(b=None), dict(f=0), dict(m=2), dict(H=3), dict(W=128), dict(s=-1)):
            kw = dict(a=C.byref(sf), f=fmt, m=1, fr=0, H=4, W=6, b=dummy, s=0)
            kw.update(case)
            head = (kw["a"], kw["f"], kw["m"], kw["fr"], kw["H"], kw["W"], kw["b"])
            r_old = old(*head, kw["s"], None)
            text_old = lib.pfnl_last_error()
            assert new(*head, 0, kw["s"], None) == r_old == -1 and lib.pfnl_last_error() == text_old, (fmt, case)


def test_the_keywords_are_checked_before_anything_touches_an_engine():
    from pfnl_amd.stream import VideoStream
    assert chroma_arguments() == (0, 0) and chroma_arguments("422") == (1, 1) and chroma_arguments("444", "420") == (2, 0)
    for bad in [("4:2:2", None), ("420", "411"), (1, None), (None, None), ("420", 2)]:
        with pytest.raises(ValueError):
            chroma_arguments(*bad)
    for kw in ({"chroma": "440"}, {"out_chroma": 2}):
        with pytest.raises(ValueError):
            VideoStream(None, 16, 24, 1, None, pixel_format="i420", **kw)
    assert frame_shapes("i420", 16, 24, "422") == frame_shapes("p010", 16, 24, "422") == ((32, 24), (768,))
    assert frame_shapes("nv12", 15, 23, "444") == ((45, 23), (1035,)) and frame_shapes("rgb24", 16, 24, "444") == ((16, 24, 3),)
    assert frame_shapes("nv12", 16, 24) == ((24, 24), (576,))
    assert output_grid("rgb24", "420") == (1, 1) and output_grid("nv12") == (2, 2) and output_grid("i010", "422") == (1, 2)
    assert output_grid("p010", "444") == (1, 1)
    assert resize_arguments((63, 96), 64, 96, "i420", "422") == (63, 96) and resize_arguments((63, 95), 64, 96, "nv12", "444") == (63, 95)
    assert resize_arguments((63, 95), 64, 96, "rgb24", "420") == (63, 95)
    for size, chroma in (((63, 96), "420"), ((64, 95), "422"), ((63, 95), "422")):
        with pytest.raises(ValueError):
            resize_arguments(size, 64, 96, "i420", chroma)
        with pytest.raises(ValueError):
            placement_arguments(size, 64, 96, "i420", fit="contain", out_chroma=chroma)
    for chroma, gx in (("422", 2), ("444", 1)):                                 # the grid per axis: (1, 2) | (1, 1)
        oH, oW, src, dst, _ = placement_arguments((45, 90), 64, 96, "i420", fit="contain", out_chroma=chroma)
        assert (oH, oW) == (45, 90) and dst[2] == 45 and dst[3] % gx == 0 and dst[1] % gx == 0 and dst[0] == 0
    # a tall canvas: 46 across, 46 * 64 / 96 = 30.67 down - 31 where the rows are on no grid, 2 * round(15.33) = 30 at 4:2:0
    assert placement_arguments((90, 46), 64, 96, "i420", fit="contain", out_chroma="422")[3] == (29, 0, 31, 46)
    assert placement_arguments((90, 46), 64, 96, "i420", fit="contain", out_chroma="444")[3] == (29, 0, 31, 46)
    assert placement_arguments((90, 46), 64, 96, "i420", fit="contain")[3] == (30, 0, 30, 46)


# ---- 7. the host-only headers as a plain C++ program ----------------------------------------------------------------------------------------------
DRIVER = r"""
#include <cstdio>
#include "stream_route.h"
int main() {
    const int sizes[4][2] = {{16, 24}, {15, 24}, {15, 23}, {1, 2}};
    for (int chroma = -1; chroma <= 3; ++chroma)
        for (int fmt = -1; fmt <= 6; ++fmt)
            for (const auto& sz : sizes) {
                const pfnl::SurfaceGeom g = pfnl::surface_geom(fmt, sz[0], sz[1], chroma);
                std::printf("G %d %d %d %d | %d %d | %d %zu | %d %zu | %d %zu\n", chroma, fmt, sz[0], sz[1], g.planes, g.sample_bytes, g.plane[0].rows,
                            g.plane[0].row_bytes, g.plane[1].rows, g.plane[1].row_bytes, g.plane[2].rows, g.plane[2].row_bytes);
            }
    const int out_sizes[4][2] = {{0, 0}, {36, 54}, {37, 54}, {37, 55}};
    for (int chroma = 0; chroma <= 2; ++chroma)
        for (int fmt = 0; fmt <= 5; ++fmt)
            for (const auto& sz : out_sizes) {
                const char* why = pfnl::route_refused(0, fmt, sz[0] ? sz[0] : 64, sz[1] ? sz[1] : 96, chroma);
                std::printf("X %d %d %d %d | %s\n", chroma, fmt, sz[0], sz[1], why ? why : "ok");
                if (why) continue;
                const pfnl::OutRoute r = pfnl::out_route(fmt, 64, 96, sz[0], sz[1], chroma);
                std::printf("R %d %d %d %d | %d %d %d | %d | %zu %zu %zu | %d | %d %d %zu\n", chroma, fmt, sz[0], sz[1], (int)r.runs[0], (int)r.runs[1],
                            (int)r.runs[2], r.sample_bytes, r.stage_bytes[0], r.stage_bytes[1], r.stage_bytes[2], r.last, r.out_h, r.out_w, r.frame_bytes);
            }
    for (int chroma = -1; chroma <= 3; chroma += 4) {
        const char* why = pfnl::route_refused(0, 2, 64, 96, chroma);
        std::printf("X %d 2 0 0 | %s\n", chroma, why ? why : "ok");
    }
    // the defaults are the calls as they were
    const pfnl::SurfaceGeom a = pfnl::surface_geom(2, 16, 24), b = pfnl::surface_geom(2, 16, 24, PFNL_CHROMA_420);
    const pfnl::OutRoute ra = pfnl::out_route(1, 64, 96, 36, 54), rb = pfnl::out_route(1, 64, 96, 36, 54, PFNL_CHROMA_420);
    std::printf("D %d %d %d\n", (int)(a.plane[1].rows == b.plane[1].rows && a.plane[2].row_bytes == b.plane[2].row_bytes),
                (int)(ra.frame_bytes == rb.frame_bytes), (int)(pfnl::route_refused(0, 1, 37, 54) == pfnl::route_refused(0, 1, 37, 54, PFNL_CHROMA_420)));
    // surface_refused with the subsampling: NV24 needs rows of 2 W samples, I422 three planes of H rows
    char mem[64];
    pfnl_surface sf{{mem, mem, mem}, {24, 24, 24}};
    const char* w1 = pfnl::surface_refused(&sf, 1, 4, 24, PFNL_CHROMA_422);
    const char* w2 = pfnl::surface_refused(&sf, 1, 4, 24, PFNL_CHROMA_444);
    const char* w3 = pfnl::surface_refused(&sf, 2, 4, 24, PFNL_CHROMA_444);
    const char* w4 = pfnl::surface_refused(&sf, 5, 4, 24, PFNL_CHROMA_422);
    const char* w5 = pfnl::surface_refused(&sf, 5, 4, 12, PFNL_CHROMA_422);
    const char* w6 = pfnl::surface_refused(&sf, 2, 4, 24, 3);
    sf.plane[2] = nullptr;
    const char* w7 = pfnl::surface_refused(&sf, 2, 4, 24, PFNL_CHROMA_444);
    const char* w8 = pfnl::surface_refused(&sf, 1, 4, 12, PFNL_CHROMA_444);
    std::printf("S %s|%s|%s|%s|%s|%s|%s|%s\n", w1 ? w1 : "ok", w2 ? w2 : "ok", w3 ? w3 : "ok", w4 ? w4 : "ok", w5 ? w5 : "ok", w6 ? w6 : "ok",
                w7 ? w7 : "ok", w8 ? w8 : "ok");
    std::printf("Y %d %d %d\n", (int)pfnl::is_yuv(0), (int)pfnl::is_yuv(2), (int)pfnl::is_yuv(5));
    return 0;
}
"""


def _build_and_run(tmp_path, name, extra=()):
    src, exe = tmp_path / "driver.cpp", tmp_path / name
    src.write_text(DRIVER)
    subprocess.run([_compiler(), "-std=c++17", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "pfnl_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout


@pytest.fixture(scope="module")
def driver_text(tmp_path_factory):
    return _build_and_run(tmp_path_factory.mktemp("chroma"), "driver")


def test_the_headers_answer_as_the_python_side_does(driver_text):
    names = {v: k for k, v in _capi.PIXEL_FORMATS.items()}
    lines = [[part.split() for part in line.split("|")] for line in driver_text.strip().split("\n")]
    seen = 0
    for parts in lines:
        if parts[0][0] == "G":
            chroma, fmt, H, W = (int(v) for v in parts[0][1:])
            planes, width = (int(v) for v in parts[1])
            geom = [(int(r), int(b)) for r, b in parts[2:]]
            try:
                want = surface.plane_shapes(names[fmt], H, W, yuv.CHROMAS[chroma]) if fmt in names and 0 <= chroma <= 2 else None
            except ValueError:
                continue                                                        # (sizes the subsampling does not take: the entries refuse them)
            if want is None:
                assert planes == 0 and width == 0 and all(g == (0, 0) for g in geom), parts
                continue
            seen += 1
            assert planes == len(want) and width == want[0][2].itemsize
            assert geom[:planes] == [(rows, n * dt.itemsize) for rows, n, dt in want], parts
        elif parts[0][0] == "R":
            chroma, fmt, oH, oW = (int(v) for v in parts[0][1:])
            name, sub = names[fmt], yuv.CHROMAS[chroma]
            out_h, out_w, frame_bytes = (int(v) for v in parts[5])
            runs = [int(v) for v in parts[1]]
            assert runs == [1, int(oH != 0), int(name in _capi.FORMATS_420)]
            assert (out_h, out_w) == ((oH, oW) if oH else (64, 96))
            assert frame_bytes == int(np.prod(frame_shapes(name, out_h, out_w, sub)[0])) * np.dtype(frame_dtype(name)).itemsize
            assert frame_bytes == [int(v) for v in parts[3]][int(parts[4][0])]
            seen += 1
    assert seen > 100
    refusals = {tuple(int(v) for v in parts[0][1:]): " ".join(parts[1]) for parts in lines if parts[0][0] == "X"}
    for (chroma, fmt, oH, oW), verdict in refusals.items():
        if not 0 <= chroma <= 2:
            assert "chroma format" in verdict
            continue
        gy, gx = output_grid(names[fmt], yuv.CHROMAS[chroma])
        assert (verdict == "ok") == (oH % gy == 0 and oW % gx == 0), (chroma, fmt, oH, oW, verdict)
        if verdict != "ok":
            assert "even" in verdict
    assert refusals[(1, 2, 37, 54)] == "ok" and "even" in refusals[(1, 2, 37, 55)] and refusals[(2, 4, 37, 55)] == "ok" and "even" in refusals[(0, 1, 37, 54)]
    assert "D 1 1 1" in driver_text and "Y 0 1 1" in driver_text
    s = next(line for line in driver_text.split("\n") if line.startswith("S "))[2:].split("|")
    assert s[0] == "ok" and "pitch" in s[1] and s[2] == "ok" and "pitch" in s[3] and s[4] == "ok" and "no plane layout" in s[5]
    assert "NULL" in s[6] and s[7] == "ok"


def test_the_driver_is_clean_under_the_sanitizers(driver_text, tmp_path):
    """a stand-alone program: the sanitizers' runtimes are linked into it, nothing is preloaded"""
    assert _build_and_run(tmp_path, "driver_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")) == driver_text


# ---- 8. Y4M and the command line -----------------------------------------------------------------------------------------------------------------
TAGS = [(b"C422", "422", 8, b"C422 XYSCSS=422"), (b"C444", "444", 8, b"C444 XYSCSS=444"), (b"C422p10", "422", 10, b"C422p10 XYSCSS=422P10"),
        (b"C444p10", "444", 10, b"C444p10 XYSCSS=444P10")]


@pytest.mark.parametrize("tag,chroma,bits,written", TAGS)
def test_the_four_tags_parsed_and_written(tag, chroma, bits, written):
    line = b"YUV4MPEG2 W6 H4 F30000:1001 Ip A1:1 " + tag + b" XYSCSS=" + tag[1:].upper() + b" XCOLORRANGE=FULL"
    with pytest.raises(ValueError, match=tag.decode()):                         # refused by name unless asked for,
        y4m.Y4MHeader.parse(line)
    with pytest.raises(ValueError, match=tag.decode()):
        y4m.Y4MHeader.parse(line, depths=(8, 10))
    with pytest.raises(ValueError, match=tag.decode()):                         # and with the wrong one asked for
        y4m.Y4MHeader.parse(line, depths=(8, 10), chromas=("420", "444" if chroma == "422" else "422"))
    if bits == 10:
        with pytest.raises(ValueError, match=tag.decode()):
            y4m.Y4MHeader.parse(line, chromas=y4m.CHROMAS)
    h = y4m.Y4MHeader.parse(line, depths=(8, 10), chromas=y4m.CHROMAS)
    assert (h.chroma, h.bits, h.siting, h.full_range, h.width, h.height) == (chroma, bits, "left", True, 6, 4)
    assert h.frame_samples == (48 if chroma == "422" else 72) and h.frame_bytes == h.frame_samples * (2 if bits == 10 else 1)
    assert h.to_bytes() == line + b"\n"
    out = h.for_output(24, 16, bits=bits)
    assert out.to_bytes() == b"YUV4MPEG2 W24 H16 F30000:1001 Ip A1:1 " + written + b" XCOLORRANGE=FULL\n"
    assert h.for_output(24, 16, bits=8, chroma="420", siting="left").to_bytes() == b"YUV4MPEG2 W24 H16 F30000:1001 Ip A1:1 C420mpeg2 XCOLORRANGE=FULL\n"
    plain = y4m.Y4MHeader.parse(b"YUV4MPEG2 W6 H4 C420jpeg XYSCSS=420JPEG")
    assert plain.chroma == "420" and plain.for_output(24, 16, bits=bits, chroma=chroma).to_bytes() == b"YUV4MPEG2 W24 H16 A1:1 " + written + b"\n"
    assert plain.for_output(24, 16).to_bytes() == b"YUV4MPEG2 W24 H16 A1:1 C420jpeg\n"


def test_sizes_and_refusals_of_the_headers():
    all_ = dict(depths=(8, 10), chromas=y4m.CHROMAS)
    assert y4m.Y4MHeader.parse(b"YUV4MPEG2 W5 H3 C444", **all_).frame_bytes == 45
    assert y4m.Y4MHeader.parse(b"YUV4MPEG2 W1 H1 C444p10", **all_).frame_bytes == 6
    assert y4m.Y4MHeader.parse(b"YUV4MPEG2 W6 H3 C422", **all_).frame_bytes == 36
    for line in (b"YUV4MPEG2 W5 H4 C422", b"YUV4MPEG2 W5 H4 C422p10", b"YUV4MPEG2 W6 H3 C420jpeg", b"YUV4MPEG2 W0 H3 C444"):
        with pytest.raises(ValueError, match="W"):
            y4m.Y4MHeader.parse(line, **all_)
    for tag in (b"Cmono", b"C411", b"C444alpha", b"C422p12", b"C444p16", b"Cmono10"):
        with pytest.raises(ValueError, match=tag.decode()):
            y4m.Y4MHeader.parse(b"YUV4MPEG2 W6 H4 " + tag, **all_)
    with pytest.raises(ValueError, match="C420jpeg"):                           # a reader that takes 4:2:2 alone
        y4m.Y4MHeader.parse(b"YUV4MPEG2 W6 H4 C420jpeg", chromas=("422",))
    with pytest.raises(ValueError):
        y4m.Y4MHeader(6, 4, chroma="440")
    assert y4m.Y4MReader(io.BytesIO(b"YUV4MPEG2 W6 H4\n")).header.chroma == "420"


@pytest.mark.parametrize("tag,chroma,bits,written", TAGS)
def test_frames_read_written_and_truncated(tag, chroma, bits, written):
    H, W = 3, 6 if chroma == "422" else 5
    rng = np.random.default_rng(3)
    n = yuv.frame_bytes(H, W, chroma)
    frames = [rng.integers(0, 1 << bits, (n // W, W)).astype(np.uint16 if bits == 10 else np.uint8) for _ in range(3)]
    head = b"YUV4MPEG2 W%d H%d " % (W, H) + tag + b"\n"
    data = head + b"".join(b"FRAME\n" + f.astype("<u2" if bits == 10 else np.uint8).tobytes() for f in frames)
    with pytest.raises(ValueError, match=tag.decode()):
        y4m.Y4MReader(io.BytesIO(data))
    reader = y4m.Y4MReader(io.BytesIO(data), depths=(8, 10), chromas=y4m.CHROMAS)
    got = list(reader)
    assert len(got) == 3 and all(g.shape == (n // W, W) and np.array_equal(g, f) for g, f in zip(got, frames))
    out = io.BytesIO()
    writer = y4m.Y4MWriter(out, reader.header)
    for f in frames:
        writer.write_frame(f.reshape(-1))
    assert out.getvalue() == b"YUV4MPEG2 W%d H%d A1:1 " % (W, H) + tag + b"\n" + data[len(head):]
    with pytest.raises(ValueError, match="samples"):
        writer.write_frame(frames[0].reshape(-1)[:H * W * 3 // 2])              # a 4:2:0 frame's worth
    for cut in (1, n * (2 if bits == 10 else 1) // 2):
        reader = y4m.Y4MReader(io.BytesIO(data[:-cut]), depths=(8, 10), chromas=y4m.CHROMAS)
        assert reader.read_frame() is not None and reader.read_frame() is not None
        with pytest.raises(ValueError, match="truncated"):
            reader.read_frame()


def test_the_two_flags():
    p = up.parser()
    base = ["in.y4m", "out.y4m", "--synthetic-weights", "0"]
    a = p.parse_args(base)
    assert a.chroma == "420" and a.out_chroma is None
    a = p.parse_args(base + ["--chroma", "any", "--out-chroma", "444"])
    assert a.chroma == "any" and a.out_chroma == "444"
    for bad in (["--chroma", "411"], ["--out-chroma", "any"], ["--chroma"]):
        with pytest.raises(SystemExit):
            p.parse_args(base + bad)


def test_a_422_stream_without_the_flag_exits_1_naming_the_tag(tmp_path, capsys):
    src = tmp_path / "in.y4m"
    src.write_bytes(b"YUV4MPEG2 W6 H4 C422\n")
    assert up.main([str(src), str(tmp_path / "out.y4m"), "--synthetic-weights", "0"]) == 1
    assert "C422" in capsys.readouterr().err
    assert up.main([str(src), str(tmp_path / "out.y4m"), "--synthetic-weights", "0", "--chroma", "444"]) == 1
    assert "C422" in capsys.readouterr().err


def test_session_keywords_derive_the_subsampling():
    all_ = dict(depths=(8, 10), chromas=y4m.CHROMAS)
    plain = up.session_keywords(y4m.Y4MHeader.parse(b"YUV4MPEG2 W24 H16 C420mpeg2"))
    assert "chroma" not in plain and "out_chroma" not in plain                  # a 4:2:0 stream: the keywords as they were
    assert "out_chroma" not in up.session_keywords(y4m.Y4MHeader.parse(b"YUV4MPEG2 W24 H16 C420mpeg2"), out_chroma=None)
    kw = up.session_keywords(y4m.Y4MHeader.parse(b"YUV4MPEG2 W24 H16 C422", **all_))
    assert kw["chroma"] == "422" and "out_chroma" not in kw and kw["chroma_siting"] == "left" and kw["out_chroma_siting"] == "left"
    kw = up.session_keywords(y4m.Y4MHeader.parse(b"YUV4MPEG2 W24 H16 C444p10", **all_), out_chroma="420", out_format="i010")
    assert (kw["chroma"], kw["out_chroma"], kw["in_depth"]) == ("444", "420", 10) and "out_chroma_siting" not in kw
    kw = up.session_keywords(y4m.Y4MHeader.parse(b"YUV4MPEG2 W24 H16 C420jpeg"), out_chroma="422")
    assert kw["chroma_siting"] == "center" and kw["out_chroma_siting"] == "left" and "chroma" not in kw
    with pytest.raises(ValueError, match="co-sited"):
        up.session_keywords(y4m.Y4MHeader.parse(b"YUV4MPEG2 W24 H16 C420jpeg"), out_chroma="422", out_chroma_siting="center")
    with pytest.raises(ValueError, match="header"):
        up.session_keywords(y4m.Y4MHeader.parse(b"YUV4MPEG2 W24 H16 C420jpeg"), chroma="422")
    with pytest.raises(ValueError, match="out_chroma"):
        up.session_keywords(y4m.Y4MHeader.parse(b"YUV4MPEG2 W24 H16 C420jpeg"), out_chroma="411")


class _StubSession:
    """open_stream's keywords noted; every pushed frame comes back as a frame of the output's size holding the input's first sample"""

    def __init__(self, H, W, batch, **kw):
        self.kw, self.H, self.W, self.scale, self.out_size = kw, H, W, 4, kw.get("out_size")
        self.out_chroma_siting = kw.get("out_chroma_siting") or kw["chroma_siting"]
        self.out_chroma = kw.get("out_chroma") or kw.get("chroma", "420")
        self.n = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return None

    def push(self, frame):
        assert frame.shape == frame_shapes("i420", self.H, self.W, self.kw.get("chroma", "420"))[0]
        oH, oW = self.out_size or (4 * self.H, 4 * self.W)
        out = np.full(frame_shapes(self.kw["out_format"], oH, oW, self.out_chroma)[0], frame.reshape(-1)[0], frame_dtype(self.kw["out_format"]))
        self.n += 1
        return [(self.n - 1, out)]

    def end(self):
        return []


def test_the_upscale_loop_around_a_stub_session():
    made = []

    def open_stream(H, W, batch, **kw):
        made.append(_StubSession(H, W, batch, **kw))
        return made[-1]

    for tag, chroma, bits, out_kw, head in ((b"C422", "422", 8, {}, b"YUV4MPEG2 W24 H16 A1:1 C422 XYSCSS=422\n"),
                                            (b"C444p10", "444", 10, {"out_format": "i010", "out_chroma": "422"},
                                             b"YUV4MPEG2 W24 H16 A1:1 C422p10 XYSCSS=422P10\n"),
                                            (b"C444", "444", 8, {"out_chroma": "420"}, b"YUV4MPEG2 W24 H16 A1:1 C420mpeg2\n"),
                                            (b"C420paldv", "420", 8, {"out_chroma": "444", "out_size": (15, 23)},
                                             b"YUV4MPEG2 W23 H15 A1:1 C444 XYSCSS=444\n")):
        H, W = 4, 6
        n = yuv.frame_bytes(H, W, chroma)
        frames = [np.full(n, 7 + k, np.uint16 if bits == 10 else np.uint8) for k in range(3)]
        data = b"YUV4MPEG2 W6 H4 " + tag + b"\n" + b"".join(b"FRAME\n" + f.astype("<u2" if bits == 10 else np.uint8).tobytes() for f in frames)
        out = io.BytesIO()
        reader = y4m.Y4MReader(io.BytesIO(data), depths=(8, 10), chromas=y4m.CHROMAS)
        assert up.upscale(reader, y4m.Y4MWriter(out), open_stream, log=io.StringIO(), **out_kw) == 3
        kw = made[-1].kw
        assert kw.get("chroma", "420") == chroma and kw.get("out_chroma") == out_kw.get("out_chroma")
        got_head, body = out.getvalue().split(b"\n", 1)
        assert got_head + b"\n" == head
        oH, oW = out_kw.get("out_size", (16, 24))
        per = yuv.frame_bytes(oH, oW, out_kw.get("out_chroma", chroma)) * (2 if out_kw.get("out_format") == "i010" else 1)
        assert len(body) == 3 * (6 + per) and body.count(b"FRAME\n") >= 3
