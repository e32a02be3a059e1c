"""10-bit output without a device: the integer rule of pfnl_amd/depth10.py - coefficients against the documented integers and the real-valued
BT.601 / BT.709 equations, the layouts, the chroma filter against a brute-force loop, the resampler's fixed point, the float32 quantisation -
and the argument checks of the C-ABI and of VideoStream that need no GPU (include/pfnl_hip.h pfnl_yuv10_coefficients, pfnl_op_quantise_u10,
pfnl_op_rgb_to_yuv420_u10, pfnl_op_resize_u10, pfnl_stream_format)."""
import ctypes as C
from fractions import Fraction
from math import lcm

import numpy as np
import pytest

from pfnl_amd import _capi, depth10, resize, yuv

PAIRS = [("bt601", False), ("bt601", True), ("bt709", False), ("bt709", True)]
TABLE = {("bt709", False): (64, (2983, 10034, 1013, -1644, -5531, 7175, 7175, -6517, -658)),
         ("bt601", False): (64, (4195, 8236, 1599, -2421, -4754, 7175, 7175, -6008, -1167)),
         ("bt709", True): (0, (3483, 11718, 1183, -1877, -6315, 8192, 8192, -7441, -751)),
         ("bt601", True): (0, (4899, 9617, 1868, -2765, -5427, 8192, 8192, -6860, -1332))}
# the nine geometries of tests/test_gpu_resize.py
GEOMETRIES = [((8, 8), (2, 2)), ((16, 24), (16, 24)), ((16, 24), (9, 13)), ((64, 96), (36, 54)), ((64, 96), (16, 24)), ((64, 96), (128, 192)),
              ((48, 80), (90, 100)), ((40, 200), (30, 75)), ((20, 600), (10, 333))]
KR_KB = {"bt601": (Fraction(299, 1000), Fraction(114, 1000)), "bt709": (Fraction(2126, 10000), Fraction(722, 10000))}   # the standards' decimals


def _constant(colour, H=2, W=2):
    return np.broadcast_to(np.asarray(colour, np.uint16), (H, W, 3)).copy()


def _yuv_of(colour, fmt, matrix, full):
    Y, Cb, Cr = depth10.planes10(depth10.from_rgb10(_constant(colour), fmt, matrix, full), fmt, 2, 2)
    assert len(np.unique(Y)) == 1
    return int(Y[0, 0]), int(Cb[0, 0]), int(Cr[0, 0])


def _blocks(rng, shape, block=2):
    """0 or 1023 in blocks of `block` samples: every clip of either direction fires next to its opposite"""
    small = rng.integers(0, 2, size=tuple((s + block - 1) // block for s in shape[:2]) + tuple(shape[2:]), dtype=np.uint16) * 1023
    return np.repeat(np.repeat(small, block, axis=0), block, axis=1)[:shape[0], :shape[1]]


# ---- 1. coefficients ---------------------------------------------------------------------------------------------------------------------
def test_coefficients_are_the_documented_integers():
    for (matrix, full), want in TABLE.items():
        assert depth10.coefficients10(matrix, full) == want
        y0, enc = want
        assert sum(enc[0:3]) == yuv._rnd(1.0 if full else 876.0 / 1023.0)
        assert sum(enc[3:6]) == 0 and sum(enc[6:9]) == 0
    for bad in ("bt2020", "BT709", None):
        with pytest.raises(ValueError):
            depth10.coefficients10(bad, False)
    assert yuv.coefficients("bt601", False)[1] == (4207, 8260, 1604, -2428, -4768, 7196, 7196, -6026, -1170)   # the 8-bit table is what it was


@pytest.mark.parametrize("fmt", depth10.FORMATS)
def test_greys_white_and_black(fmt):
    for matrix, full in PAIRS:
        assert _yuv_of((1023, 1023, 1023), fmt, matrix, full) == ((1023 if full else 940), 512, 512)
        assert _yuv_of((0, 0, 0), fmt, matrix, full) == ((0 if full else 64), 512, 512)
    g = np.arange(1024, dtype=np.uint16)
    ramp = np.repeat(np.stack([g, g, g], axis=-1)[None], 2, axis=0)            # [2, 1024, 3]: every grey, next to its neighbours
    for matrix, full in PAIRS:
        Y, Cb, Cr = depth10.planes10(depth10.from_rgb10(ramp, fmt, matrix, full), fmt, 2, 1024)
        assert (Cb == 512).all() and (Cr == 512).all()
        if full:
            assert np.array_equal(Y[0], g)
        for v in (0, 1, 511, 1023):
            assert _yuv_of((v, v, v), fmt, matrix, full)[1:] == (512, 512)


# ---- 2. the real-valued equations --------------------------------------------------------------------------------------------------------
def _exact_rows(matrix, full):
    """y0 and the three rows of the real-valued equations as Fractions: Y = y0 + row0 . RGB, Cb = 512 + row1 . RGB, Cr = 512 + row2 . RGB"""
    kr, kb = KR_KB[matrix]
    kg = 1 - kr - kb
    ys, cs = (Fraction(1), Fraction(1)) if full else (Fraction(876, 1023), Fraction(896, 1023))
    y = (ys * kr, ys * kg, ys * kb)
    cb = tuple(cs * v / (2 * (1 - kb)) for v in (-kr, -kg, 1 - kb))
    cr = tuple(cs * v / (2 * (1 - kr)) for v in (1 - kr, -kg, -kb))
    return (0 if full else 64), (y, cb, cr)


@pytest.mark.parametrize("matrix,full", PAIRS)
def test_constant_colours_are_within_the_coefficients_error_of_the_real_equations(matrix, full):
    """|int - real| <= 0.5 + 1023 sum |c_int / 2^14 - c_exact| per row: the one rounding, and the coefficients' own error times the largest
    sample.  The real value is formed exactly (integers over the rows' common denominator)."""
    lattice = list(range(0, 1024, 33))
    assert lattice[-1] == 1023 and len(lattice) == 32
    colours = np.array([(r, g, b) for r in lattice for g in lattice for b in lattice] +
                       [(r, g, b) for r in (0, 1023) for g in (0, 1023) for b in (0, 1023)], np.int64)
    n = len(colours)
    # every colour as a constant frame: in a frame of two rows, a colour that fills the columns 4b .. 4b + 3 owns the chroma sample at column
    # 4b + 2 (its taps are the columns 4b + 1 .. 4b + 3, both rows) and every luma sample of its block
    frames = np.broadcast_to(colours.astype(np.uint16)[None, :, None, :], (2, n, 4, 3)).reshape(2, 4 * n, 3)
    Y, Cb, Cr = depth10.planes10(depth10.from_rgb10(frames, "i010", matrix, full), "i010", 2, 4 * n)
    assert np.array_equal(Y[0], Y[1]) and np.array_equal(Y[0, 0::4], Y[0, 3::4])
    for k in (0, n - 1):                                                        # (and that is what a 2 x 2 frame of the colour gives)
        assert _yuv_of(tuple(colours[k]), "i010", matrix, full) == (int(Y[0, 4 * k]), int(Cb[0, 2 * k + 1]), int(Cr[0, 2 * k + 1]))
    y0, enc = depth10.coefficients10(matrix, full)
    off, rows = _exact_rows(matrix, full)
    assert off == y0
    R, G, B = (colours[:, k] for k in range(3))
    for name, base, got, c_int, c_exact in (("Y", y0, Y[0, 0::4], enc[0:3], rows[0]), ("Cb", 512, Cb[0, 1::2], enc[3:6], rows[1]),
                                            ("Cr", 512, Cr[0, 1::2], enc[6:9], rows[2])):
        bound = Fraction(1, 2) + 1023 * sum(abs(Fraction(ci, 1 << 14) - ce) for ci, ce in zip(c_int, c_exact))
        L = lcm(*(ce.denominator for ce in c_exact))
        A = [int(ce * L) for ce in c_exact]
        assert all(Fraction(a, L) == ce for a, ce in zip(A, c_exact))
        assert (base + 1023) * L + 1023 * sum(abs(a) for a in A) < (1 << 62)
        real_L = base * L + A[0] * R + A[1] * G + A[2] * B                      # the real value times L, exactly
        unclipped = base + ((c_int[0] * R + c_int[1] * G + c_int[2] * B + (1 << 13)) >> 14)
        act = (unclipped < 0) | (unclipped > 1023)                              # where the clip acts: full-range chroma of saturated blue / red
        assert not act.any() if (name == "Y" or not full) else act.sum() <= 64
        got = got.astype(np.int64)
        assert np.array_equal(got, np.clip(unclipped, 0, 1023))
        worst = int(np.abs(got * L - real_L)[~act].max())
        assert Fraction(worst, L) <= bound, (name, float(Fraction(worst, L)), float(bound))
        assert bound < Fraction(6, 10)                                          # (each coefficient is good to 2^-15, the derived one to 2^-14)


# ---- 3. the layouts ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(2, 2), (4, 6), (6, 4)])
def test_layouts_hold_the_same_planes(H, W):
    rng = np.random.default_rng(7)
    rgb = rng.integers(0, 1024, (H, W, 3), dtype=np.uint16)
    p010, i010 = depth10.from_rgb10(rgb, "p010"), depth10.from_rgb10(rgb, "i010")
    assert p010.shape == i010.shape == (H * 3 // 2, W) and p010.dtype == i010.dtype == np.uint16
    assert not (p010 & 63).any()
    for a, b in zip(depth10.planes10(p010, "p010", H, W), depth10.planes10(i010, "i010", H, W)):
        assert np.array_equal(a, b)
    Y, Cb, Cr = depth10.planes10(i010, "i010", H, W)
    flat = p010.reshape(-1) >> 6
    assert np.array_equal(flat[:H * W], Y.reshape(-1))
    assert np.array_equal(flat[H * W::2], Cb.reshape(-1)) and np.array_equal(flat[H * W + 1::2], Cr.reshape(-1))
    assert np.array_equal(i010.reshape(-1)[H * W:H * W * 5 // 4], Cb.reshape(-1)) and np.array_equal(i010.reshape(-1)[H * W * 5 // 4:], Cr.reshape(-1))
    for fmt in depth10.FORMATS:
        x = (rng.integers(0, 1024, (H * W * 3 // 2,), dtype=np.uint16) << depth10.SHIFT[fmt]).astype(np.uint16)   # any in-range samples are a frame
        assert np.array_equal(depth10.pack10(*depth10.planes10(x, fmt, H, W), fmt).reshape(-1), x)
    with pytest.raises(ValueError):
        depth10.planes10(i010, "i010", H + 1, W)
    with pytest.raises(ValueError):
        depth10.planes10(i010, "nv12", H, W)
    with pytest.raises(ValueError):
        depth10.from_rgb10(rgb, "i420")
    bad = i010.copy()
    bad[0, 0] = 1024
    with pytest.raises(ValueError):
        depth10.planes10(bad, "i010", H, W)
    bad = p010.copy()
    bad[0, 0] |= 1
    with pytest.raises(ValueError):
        depth10.planes10(bad, "p010", H, W)
    with pytest.raises(ValueError):
        depth10.pack10(np.full((H, W), 1024), Cb, Cr, "i010")
    over = rgb.copy()
    over[0, 0, 0] = 1024
    with pytest.raises(ValueError):
        depth10.from_rgb10(over, "p010")
    with pytest.raises(ValueError):
        depth10.from_rgb10(np.zeros((3, 4, 3), np.uint16), "p010")
    with pytest.raises(ValueError):
        depth10.from_rgb10(np.zeros((4, 5, 3), np.uint16), "i010")
    with pytest.raises(ValueError):
        depth10.from_rgb10(np.zeros((4, 4, 3), np.uint8), "i010")


# ---- 4. the chroma filter ----------------------------------------------------------------------------------------------------------------
def _brute_force(rgb, matrix, full):
    """from_rgb10's three planes in Python integers, sample by sample"""
    H, W = rgb.shape[:2]
    y0, (yr, yg, yb, cbr, cbg, cbb, crr, crg, crb) = depth10.coefficients10(matrix, full)
    px = [[tuple(int(v) for v in rgb[y, x]) for x in range(W)] for y in range(H)]
    Y = [[min(max((yr * r + yg * g + yb * b + (y0 << 14) + (1 << 13)) >> 14, 0), 1023) for r, g, b in row] for row in px]
    planes = []
    for cr_, cg_, cb_ in ((cbr, cbg, cbb), (crr, crg, crb)):
        plane = []
        for j in range(H // 2):
            line = []
            for i in range(W // 2):
                S = 0
                for y in (2 * j, 2 * j + 1):
                    for x, wgt in ((2 * i - 1, 1), (2 * i, 2), (2 * i + 1, 1)):
                        r, g, b = px[y][min(max(x, 0), W - 1)]
                        S += wgt * (cr_ * r + cg_ * g + cb_ * b)
                assert abs(S) + (512 << 17) + (1 << 16) < (1 << 31)
                line.append(min(max(512 + ((S + (1 << 16)) >> 17), 0), 1023))
            plane.append(line)
        planes.append(plane)
    return np.array(Y), np.array(planes[0]), np.array(planes[1])


def test_chroma_filter_is_1_2_1_over_two_rows_against_a_brute_force_loop():
    rng = np.random.default_rng(11)
    frames = [rng.integers(0, 1024, (6, 10, 3), dtype=np.uint16), _blocks(rng, (6, 10, 3))]
    for x in (0, 1, 4, 9):                                                      # one column of full blue on black: the taps, and the left clamp
        f = np.zeros((6, 10, 3), np.uint16)
        f[:, x, 2] = 1023
        frames.append(f)
    for f in frames:
        for matrix, full in PAIRS:
            got = depth10.planes10(depth10.from_rgb10(f, "i010", matrix, full), "i010", 6, 10)
            for g, w in zip(got, _brute_force(f, matrix, full)):
                assert np.array_equal(g, w)
    # the impulse's weights through the filter, full range BT.709: cbb = 8192 = 1/2, so a weight w of 8 gives 512 + round(1023 w / 16)
    f = np.zeros((2, 10, 3), np.uint16)
    f[:, 4, 2] = 1023
    cb = depth10.planes10(depth10.from_rgb10(f, "i010", "bt709", True), "i010", 2, 10)[1][0]
    assert list(cb) == [512, 512, 512 + 256, 512, 512]                          # column 4 = 2 i at i = 2: 2 rows x weight 2 of 8 = 1/2 of 511.5 -> 256
    f = np.zeros((2, 10, 3), np.uint16)
    f[:, 0, 2] = 1023
    cb = depth10.planes10(depth10.from_rgb10(f, "i010", "bt709", True), "i010", 2, 10)[1][0]
    assert list(cb) == [512 + 384, 512, 512, 512, 512]                          # column -1 clamps onto column 0: weight 1 + 2 of 4 per row


# ---- 5. the resampler --------------------------------------------------------------------------------------------------------------------
def test_resize10_identity_and_flat_frames():
    rng = np.random.default_rng(3)
    f = rng.integers(0, 1024, (16, 24, 3), dtype=np.uint16)
    assert np.array_equal(depth10.resize10(f, 16, 24), f)
    for v in (0, 1, 777, 1023):
        for (H, W), (oH, oW) in GEOMETRIES[:5]:
            out = depth10.resize10(np.full((H, W, 3), v, np.uint16), oH, oW)
            assert out.shape == (oH, oW, 3) and out.dtype == np.uint16 and (out == v).all()
    with pytest.raises(ValueError):
        depth10.resize10(np.full((4, 4, 3), 1024, np.uint16), 4, 4)
    with pytest.raises(ValueError):
        depth10.resize10(np.zeros((4, 4, 3), np.uint8), 4, 4)
    # the 8-bit rule returns what it returned
    g = rng.integers(0, 256, (16, 24, 3), dtype=np.uint8)
    assert np.array_equal(resize.resize(g, 16, 24), g)


@pytest.mark.parametrize("size,out", GEOMETRIES)
def test_resize10_fixed_point_stays_inside_its_words_on_block_frames(size, out):
    (H, W), (oH, oW) = size, out
    frame = _blocks(np.random.default_rng(H * 1000 + W), (H, W, 3))
    h, v = depth10.resize10_passes(frame, oH, oW)
    assert int(np.abs(h).max()) < (1 << 15)                                     # the intermediate is an int16
    assert int(np.abs(v).max()) + (1 << 17) < (1 << 31)                         # the second sum and its rounding are an int32
    raw, got = depth10.resize10_unclipped(frame, oH, oW), depth10.resize10(frame, oH, oW)
    assert np.array_equal(got, np.clip(raw, 0, 1023))
    if (H, W) != (oH, oW) and H * W >= 256:
        assert raw.min() < 0 and raw.max() > 1023
        assert got.min() == 0 and got.max() == 1023


# ---- 6. the quantisation -----------------------------------------------------------------------------------------------------------------
def test_quantise10_edges():
    x = np.array([0.0, -0.0, 1.0, -1.0, -1e-9, 2.0, 1e30, np.inf, -np.inf, 0.5 / 1023, 1.5 / 1023, 0.5], np.float32)
    got = depth10.quantise10(x)
    assert got.dtype == np.uint16
    f32 = lambda v: float(np.float32(np.float32(v) * np.float32(1023)))          # noqa: E731
    assert list(got[:9]) == [0, 0, 1023, 0, 0, 1023, 1023, 1023, 0]
    assert list(got[9:]) == [int(np.round(f32(0.5 / 1023))), int(np.round(f32(1.5 / 1023))), 512]   # 511.5 is a tie: half to even
    assert depth10.quantise10(np.float64(0.25)) == 256                          # (255.75) any float input is taken as float32
    assert depth10.quantise10(np.zeros((2, 3, 4), np.float32)).shape == (2, 3, 4)


def test_quantise10_follows_the_float32_product():
    x = np.random.default_rng(0).random(2_000_000, dtype=np.float32)
    exact = x.astype(np.float64) * 1023.0                                       # 24 x 10 bits: the exact product
    as_f32 = np.rint(exact.astype(np.float32).astype(np.float64))               # rounded once to float32 = the float32 product, then half to even
    as_f64 = np.rint(exact)
    differ = as_f32 != as_f64
    assert 0 < int(differ.sum()) < 200                                          # there are some (about 15 per million)
    got = depth10.quantise10(x).astype(np.float64)
    assert np.array_equal(got[differ], as_f32[differ]) and np.array_equal(got, as_f32)


# ---- 7. the library, without a device ----------------------------------------------------------------------------------------------------
def test_library_coefficients_equal_the_host_rule():
    lib = _capi.load_library()
    for matrix, full in PAIRS:
        out = (C.c_int32 * 10)()
        assert lib.pfnl_yuv10_coefficients(_capi.YUV_MATRICES[matrix], int(full), out) == 0
        y0, enc = depth10.coefficients10(matrix, full)
        assert list(out) == [y0, *enc]
    out = (C.c_int32 * 10)()
    assert lib.pfnl_yuv10_coefficients(2, 0, out) == -1 and b"matrix" in lib.pfnl_last_error()
    assert lib.pfnl_yuv10_coefficients(0, 2, out) == -1 and b"full_range" in lib.pfnl_last_error()
    assert lib.pfnl_yuv10_coefficients(0, 0, None) == -1 and b"NULL" in lib.pfnl_last_error()
    assert lib.pfnl_version() == 4                                              # symbols were added, nothing changed
    assert (_capi.PIXEL_FORMATS["rgb10"], _capi.PIXEL_FORMATS["p010"], _capi.PIXEL_FORMATS["i010"]) == (3, 4, 5)


def test_op_hooks_and_stream_format_refuse_bad_arguments_without_a_device():
    lib = _capi.load_library()
    dummy = C.c_void_p(16)                                                      # never dereferenced: the hooks return first
    call = lambda src, fmt, m, fr, n, H, W, dst: lib.pfnl_op_rgb_to_yuv420_u10(src, fmt, m, fr, n, H, W, dst, None)   # noqa: E731
    assert call(None, 4, 1, 0, 1, 16, 24, dummy) == -1 and b"NULL" in lib.pfnl_last_error()
    assert call(dummy, 4, 1, 0, 1, 16, 24, None) == -1 and b"NULL" in lib.pfnl_last_error()
    for fmt in (0, 1, 2, 3, 6, -1):                                             # the 8-bit formats and RGB10 are no 10-bit 4:2:0 format
        assert call(dummy, fmt, 1, 0, 1, 16, 24, dummy) == -1 and b"fmt" in lib.pfnl_last_error()
    assert call(dummy, 4, 2, 0, 1, 16, 24, dummy) == -1 and b"matrix" in lib.pfnl_last_error()
    assert call(dummy, 5, 1, 2, 1, 16, 24, dummy) == -1 and b"full_range" in lib.pfnl_last_error()
    for H, W in ((15, 24), (16, 23), (0, 24), (16, -2)):
        assert call(dummy, 5, 0, 1, 1, H, W, dummy) == -1 and b"even" in lib.pfnl_last_error()
    assert call(dummy, 5, 0, 1, 0, 16, 24, dummy) == -1 and b"n >= 1" in lib.pfnl_last_error()
    q = lib.pfnl_op_quantise_u10
    assert q(None, dummy, 4, None) == -1 and b"NULL" in lib.pfnl_last_error()
    assert q(dummy, None, 4, None) == -1 and b"NULL" in lib.pfnl_last_error()
    for n in (0, 3, 6):
        assert q(dummy, dummy, n, None) == -1 and b"multiple of 4" in lib.pfnl_last_error()
    r = lib.pfnl_op_resize_u10
    assert r(None, 1, 16, 24, 9, 13, dummy, None) == -1 and b"NULL" in lib.pfnl_last_error()
    assert r(dummy, 1, 16, 24, 9, 13, None, None) == -1 and b"NULL" in lib.pfnl_last_error()
    assert r(dummy, 0, 16, 24, 9, 13, dummy, None) == -1 and b"n >= 1" in lib.pfnl_last_error()
    for H, W, oH, oW in ((16, 24, 3, 13), (16, 24, 9, 49), (0, 24, 9, 13), (16, 24, 0, 0), (16, -24, 9, 13), (16, 24, 9, 20000)):
        assert r(dummy, 1, H, W, oH, oW, dummy, None) == -1 and b"resize" in lib.pfnl_last_error()
    assert lib.pfnl_stream_format(None, 0, 4, 1, 0) == -1 and b"NULL" in lib.pfnl_last_error()
    # the 8-bit hooks go on refusing the new formats
    for op in (lib.pfnl_op_yuv420_to_rgb_u8, lib.pfnl_op_rgb_to_yuv420_u8):
        for fmt in (3, 4, 5):
            assert op(dummy, fmt, 1, 0, 1, 16, 24, dummy, None) == -1 and b"fmt" in lib.pfnl_last_error()


def test_video_stream_checks_its_10_bit_arguments_before_it_touches_the_engine():
    from pfnl_amd.stream import VideoStream, format_arguments, frame_dtype, frame_shapes, resize_arguments
    assert format_arguments("rgb24", "p010") == (0, 4, 1, 0)
    assert format_arguments("rgb24", "rgb10", "bt601", True) == (0, 3, 0, 1)
    assert format_arguments("nv12", "p010") == (1, 4, 1, 0) and format_arguments("i420", "i010") == (2, 5, 1, 0)
    assert format_arguments() == (0, 0, 1, 0) and format_arguments("nv12") == (1, 1, 1, 0)   # the 8-bit answers are what they were
    for kw in ({"pixel_format": "p010"}, {"pixel_format": "i010"}, {"pixel_format": "rgb10"}, {"pixel_format": "i010", "out_format": "rgb24"},
               {"pixel_format": "nv12", "out_format": "rgb10"}, {"out_format": "P010"}, {"out_format": "p010", "matrix": "bt2020"}):
        with pytest.raises(ValueError):
            format_arguments(**kw)
        with pytest.raises(ValueError):                                         # no engine is needed to hear about it
            VideoStream(None, 16, 24, 1, None, **kw)
    assert frame_shapes("rgb10", 16, 24) == ((16, 24, 3),)
    assert frame_shapes("p010", 16, 24) == frame_shapes("i010", 16, 24) == ((24, 24), (576,))
    assert frame_shapes("rgb24", 16, 24) == ((16, 24, 3),) and frame_shapes("nv12", 16, 24) == ((24, 24), (576,))
    assert [frame_dtype(f) for f in ("rgb24", "nv12", "i420", "rgb10", "p010", "i010")] == [np.uint8] * 3 + [np.uint16] * 3
    for fmt in ("p010", "i010"):
        for bad in ((37, 54), (36, 55)):
            with pytest.raises(ValueError):
                resize_arguments(bad, 64, 96, fmt)
        assert resize_arguments((36, 54), 64, 96, fmt) == (36, 54)
    assert resize_arguments((37, 55), 64, 96, "rgb10") == (37, 55)              # RGB has no chroma planes to halve
