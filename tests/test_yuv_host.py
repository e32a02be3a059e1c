"""YUV 4:2:0 without a device: the integer rule of pfnl_amd/yuv.py against known answers and against the standards' real-valued formulas
over all 2^24 colours, its two filters and two layouts, the library's coefficient table, and the argument checks of the C-ABI and of
VideoStream that need no GPU (include/pfnl_hip.h pfnl_stream_format, pfnl_op_yuv420_to_rgb_u8, pfnl_op_rgb_to_yuv420_u8)."""
import ctypes as C

import numpy as np
import pytest

from pfnl_amd import _capi, yuv

PAIRS = [("bt601", False), ("bt601", True), ("bt709", False), ("bt709", True)]


def _constant_rgb(colour, H=4, W=4):
    return np.broadcast_to(np.asarray(colour, np.uint8), (H, W, 3)).copy()


def _yuv_of(colour, fmt, matrix, full_range, H=4, W=4):
    """(Y, Cb, Cr) of a constant-colour frame, after checking that every sample of each plane agrees"""
    Y, Cb, Cr = yuv.planes(yuv.from_rgb(_constant_rgb(colour, H, W), fmt, matrix, full_range), fmt, H, W)
    assert len(np.unique(Y)) == len(np.unique(Cb)) == len(np.unique(Cr)) == 1
    return int(Y[0, 0]), int(Cb[0, 0]), int(Cr[0, 0])


# ---- 1. known answers ---------------------------------------------------------------------------------------------------------------
def test_coefficients_of_bt601_limited_are_the_documented_integers():
    y0, enc, dec = yuv.coefficients("bt601", False)
    assert y0 == 16
    assert enc == (4207, 8260, 1604, -2428, -4768, 7196, 7196, -6026, -1170)
    assert dec == (19077, 26149, -6419, -13320, 33050)
    for matrix, full in PAIRS:
        y0, enc, _ = yuv.coefficients(matrix, full)
        assert sum(enc[0:3]) == yuv._rnd(1.0 if full else 219.0 / 255.0)        # white is y0 + round(255 ys) ...
        assert sum(enc[3:6]) == 0 and sum(enc[6:9]) == 0                       # ... and greys have no chroma, exactly
    with pytest.raises(ValueError):
        yuv.coefficients("bt2020", False)


@pytest.mark.parametrize("fmt", yuv.FORMATS)
def test_known_answers_on_constant_frames(fmt):
    assert _yuv_of((255, 0, 0), fmt, "bt601", False) == (81, 90, 240)
    assert _yuv_of((255, 255, 255), fmt, "bt601", False) == (235, 128, 128)
    assert _yuv_of((0, 0, 0), fmt, "bt601", False) == (16, 128, 128)
    assert _yuv_of((255, 0, 0), fmt, "bt709", False) == (63, 102, 240)
    for matrix in ("bt601", "bt709"):
        for g in range(256):                                                   # full range: greys are exact, both ways
            assert _yuv_of((g, g, g), fmt, matrix, True, 2, 2) == (g, 128, 128)
            frame = yuv.pack(np.full((2, 2), g), np.full((1, 1), 128), np.full((1, 1), 128), fmt)
            assert np.array_equal(yuv.to_rgb(frame, fmt, 2, 2, matrix, True), _constant_rgb((g, g, g), 2, 2))


# ---- 2. the standards' formulas, all 2^24 colours -----------------------------------------------------------------------------------
def _real_constants(matrix, full):
    kr, kb = yuv.MATRICES[matrix]
    return (kr, 1.0 - kr - kb, kb) + ((0.0, 1.0, 1.0) if full else (16.0, 219.0 / 255.0, 224.0 / 255.0))


def _half_up(x):
    return np.clip(np.floor(x + 0.5), 0, 255).astype(np.int32)


@pytest.mark.parametrize("matrix,full", PAIRS)
def test_rgb_to_yuv_is_within_one_code_of_the_real_formula(matrix, full):
    """Every colour as a constant frame: in a frame of two rows, a colour that fills the columns 4b .. 4b + 3 owns the chroma sample at
    column 4b + 2 (its taps are the columns 4b + 1 .. 4b + 3, both rows) and every luma sample of its block.  The coefficients are off by
    at most 2^-15 each, so the integer numerator is within 3 * 255 * 2^-15 < 0.04 code of the real one before the one rounding: the two
    roundings differ by at most 1."""
    kr, kg, kb, y0, ys, cs = _real_constants(matrix, full)
    gb = np.arange(1 << 16)
    worst = 0
    for r in range(256):
        colours = np.stack([np.full_like(gb, r), gb >> 8, gb & 255], axis=-1).astype(np.uint8)     # [65536, 3]
        rgb = np.broadcast_to(colours[None, :, None, :], (2, 1 << 16, 4, 3)).reshape(2, 1 << 18, 3)
        Y, Cb, Cr = yuv.planes(yuv.from_rgb(rgb, "i420", matrix, full), "i420", 2, 1 << 18)
        R, G, B = (colours[:, k].astype(np.float64) for k in range(3))
        yf = kr * R + kg * G + kb * B
        want = (_half_up(y0 + ys * yf), _half_up(128.0 + cs * (B - yf) / (2.0 * (1.0 - kb))), _half_up(128.0 + cs * (R - yf) / (2.0 * (1.0 - kr))))
        got = (Y[0, 1::4], Cb[0, 1::2], Cr[0, 1::2])
        assert np.array_equal(Y[0, 0::4], Y[1, 3::4])
        worst = max(worst, max(int(np.abs(g.astype(np.int32) - w).max()) for g, w in zip(got, want)))
    assert worst <= 1, worst


@pytest.mark.parametrize("matrix,full", PAIRS)
def test_yuv_to_rgb_is_within_one_code_of_the_real_formula(matrix, full):
    """Every (Y, Cb, Cr) as a constant frame: with two luma rows there is one chroma row, onto which every vertical index clamps, and a
    colour that fills the luma columns 2b, 2b + 1 is alone in the even column 2b (taps: chroma sample b only)."""
    kr, kg, kb, y0, ys, cs = _real_constants(matrix, full)
    cc = np.arange(1 << 16)
    cb, cr = (cc >> 8).astype(np.uint8), (cc & 255).astype(np.uint8)
    U, V = (cb.astype(np.float64) - 128.0) / cs, (cr.astype(np.float64) - 128.0) / cs
    worst = 0
    for y in range(256):
        frame = yuv.pack(np.full((2, 1 << 17), y, np.uint8), cb[None, :], cr[None, :], "i420")
        got = yuv.to_rgb(frame, "i420", 2, 1 << 17, matrix, full)[0, 0::2].astype(np.int32)       # [65536, 3]
        yn = (y - y0) / ys
        want = np.stack([_half_up(yn + 2.0 * (1.0 - kr) * V),
                         _half_up(yn - 2.0 * kb * (1.0 - kb) / kg * U - 2.0 * kr * (1.0 - kr) / kg * V),
                         _half_up(yn + 2.0 * (1.0 - kb) * U)], axis=-1)
        worst = max(worst, int(np.abs(got - want).max()))
    assert worst <= 1, worst


# ---- 3. the filters -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(2, 2), (2, 6), (6, 2), (6, 10)])
def test_constant_chroma_passes_both_filters_unchanged(H, W):
    rng = np.random.default_rng(H * 100 + W)
    for c in (0, 1, 77, 128, 254, 255):
        assert np.array_equal(yuv.upsample(np.full((H // 2, W // 2), c, np.uint8), H, W), np.full((H, W), c))
    # an RGB frame built from constant chroma (and any luma) has that chroma: full range, where the round trip has room
    for cb, cr in ((128, 128), (100, 160), (140, 90)):
        Y = rng.integers(80, 177, size=(H, W), dtype=np.uint8)
        frame = yuv.pack(Y, np.full((H // 2, W // 2), cb), np.full((H // 2, W // 2), cr), "nv12")
        rgb = yuv.to_rgb(frame, "nv12", H, W, "bt709", True)
        assert rgb.min() > 0 and rgb.max() < 255                                # nothing clipped: the chroma is still in there
        _, Cb, Cr = yuv.planes(yuv.from_rgb(rgb, "nv12", "bt709", True), "nv12", H, W)
        assert np.abs(Cb.astype(int) - cb).max() <= 1 and np.abs(Cr.astype(int) - cr).max() <= 1   # (RGB was rounded to 8 bits in between)
        if (cb, cr) == (128, 128):
            assert np.all(Cb == 128) and np.all(Cr == 128)                      # greys: exact


def test_upsampling_spreads_one_sample_with_the_documented_weights():
    C = np.zeros((3, 3), np.uint8)
    C[1, 1] = 8 * 16                                                            # 128: every weight / 8 is exact
    up = yuv.upsample(C, 6, 6)
    want = np.zeros((6, 6), np.int32)
    # luma rows 2, 3 are nearest to chroma row 1 (weight 3 of 4); rows 1 and 4 see it as their far row (1 of 4).  Column 2 is co-sited
    # (x 2 of 2), columns 1 and 3 lie between two samples (1 of 2): in eighths, 6/2 on the even column and 3/1 on the odd ones.
    for y, wy in ((1, 1), (2, 3), (3, 3), (4, 1)):
        for x, wx in ((1, 1), (2, 2), (3, 1)):
            want[y, x] = 16 * wy * wx
    assert np.array_equal(up, want)
    # an odd column at the right edge clamps onto the last sample: both taps are that sample
    C = np.zeros((1, 2), np.uint8)
    C[0, 1] = 200
    assert list(yuv.upsample(C, 2, 4)[0]) == [0, 100, 200, 200]


def test_downsampling_taps_are_1_2_1_over_two_rows():
    one = 1 << (yuv.F + 3)                                                      # a numerator sum worth one code
    for y in range(2):
        for x in range(8):                                                      # chroma sample i: columns 2i - 1, 2i, 2i + 1 of rows 0, 1
            N = np.zeros((2, 8), np.int32)
            N[y, x] = 8 * one
            taps = [{2 * i - 1: 1, 2 * i: 2, 2 * i + 1: 1}.get(x, 0) + (1 if x == 0 and i == 0 else 0) for i in range(4)]
            assert list(yuv.downsample(N)[0]) == [128 + 8 * w for w in taps], (y, x)
    N = np.zeros((2, 4), np.int32)
    N[0, 0] = 8 * one                                                           # column -1 clamps onto column 0: weight 1 + 2
    assert list(yuv.downsample(N)[0]) == [128 + 24, 128]
    N = np.full((2, 2), -one // 16 - 1, np.int32)                               # S = 8 N: just below - 1/2 code rounds down (arithmetic shift)
    assert int(yuv.downsample(N)[0, 0]) == 127
    assert int(yuv.downsample(np.full((2, 2), -one // 16, np.int32))[0, 0]) == 128   # ... and - 1/2 itself rounds up


# ---- 4. the layouts --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(2, 2), (4, 6), (6, 4)])
def test_layouts_hold_the_same_planes(H, W):
    rng = np.random.default_rng(7)
    Y, Cb, Cr = rng.integers(0, 256, (H, W), np.uint8), rng.integers(0, 256, (H // 2, W // 2), np.uint8), rng.integers(0, 256, (H // 2, W // 2), np.uint8)
    nv12, i420 = yuv.pack(Y, Cb, Cr, "nv12"), yuv.pack(Y, Cb, Cr, "i420")
    assert nv12.shape == i420.shape == (H * 3 // 2, W) and nv12.dtype == np.uint8
    assert np.array_equal(np.sort(nv12.reshape(-1)), np.sort(i420.reshape(-1)))
    assert np.array_equal(nv12.reshape(-1)[H * W::2], Cb.reshape(-1)) and np.array_equal(nv12.reshape(-1)[H * W + 1::2], Cr.reshape(-1))
    assert np.array_equal(i420.reshape(-1)[H * W:H * W * 5 // 4], Cb.reshape(-1)) and np.array_equal(i420.reshape(-1)[H * W * 5 // 4:], Cr.reshape(-1))
    for fmt, frame in (("nv12", nv12), ("i420", i420)):
        for p, q in zip(yuv.planes(frame, fmt, H, W), (Y, Cb, Cr)):
            assert np.array_equal(p, q)
        x = rng.integers(0, 256, (H * W * 3 // 2,), np.uint8)                   # any bytes are a frame
        assert np.array_equal(yuv.pack(*yuv.planes(x, fmt, H, W), fmt).reshape(-1), x)
        assert np.array_equal(yuv.to_rgb(frame, fmt, H, W), yuv.to_rgb(nv12, "nv12", H, W))
    with pytest.raises(ValueError):
        yuv.planes(nv12, "nv12", H + 1, W)
    with pytest.raises(ValueError):
        yuv.planes(nv12, "yv12", H, W)
    with pytest.raises(ValueError):
        yuv.from_rgb(np.zeros((3, 4, 3), np.uint8), "nv12")


# ---- 5. the library, without a device ---------------------------------------------------------------------------------------------------
def test_library_coefficients_equal_the_host_rule():
    lib = _capi.load_library()
    for matrix, full in PAIRS:
        out = (C.c_int32 * 15)()
        assert lib.pfnl_yuv_coefficients(_capi.YUV_MATRICES[matrix], int(full), out) == 0
        y0, enc, dec = yuv.coefficients(matrix, full)
        assert list(out) == [y0, *enc, *dec]
    out = (C.c_int32 * 15)()
    assert lib.pfnl_yuv_coefficients(2, 0, out) == -1 and b"matrix" in lib.pfnl_last_error()
    assert lib.pfnl_yuv_coefficients(0, 2, out) == -1
    assert lib.pfnl_yuv_coefficients(0, 0, None) == -1 and b"NULL" in lib.pfnl_last_error()
    assert lib.pfnl_version() == 4                                              # symbols were added, nothing changed


def test_op_hooks_and_stream_format_refuse_bad_arguments_without_a_device():
    lib = _capi.load_library()
    dummy = C.c_void_p(16)                                                      # never dereferenced: the hooks return first
    for op in (lib.pfnl_op_yuv420_to_rgb_u8, lib.pfnl_op_rgb_to_yuv420_u8):
        call = lambda src, fmt, m, fr, n, H, W, dst: op(src, fmt, m, fr, n, H, W, dst, None)   # noqa: E731
        assert call(None, 1, 1, 0, 1, 16, 24, dummy) == -1 and b"NULL" in lib.pfnl_last_error()
        assert call(dummy, 1, 1, 0, 1, 16, 24, None) == -1 and b"NULL" in lib.pfnl_last_error()
        assert call(dummy, 0, 1, 0, 1, 16, 24, dummy) == -1 and b"fmt" in lib.pfnl_last_error()        # RGB24 is no 4:2:0 format
        assert call(dummy, 3, 1, 0, 1, 16, 24, dummy) == -1 and b"fmt" in lib.pfnl_last_error()
        assert call(dummy, 1, 2, 0, 1, 16, 24, dummy) == -1 and b"matrix" in lib.pfnl_last_error()
        assert call(dummy, 1, 1, 2, 1, 16, 24, dummy) == -1 and b"full_range" in lib.pfnl_last_error()
        for H, W in ((15, 24), (16, 23), (0, 24), (16, -2)):
            assert call(dummy, 2, 0, 1, 1, H, W, dummy) == -1 and b"even" in lib.pfnl_last_error()
        assert call(dummy, 2, 0, 1, 0, 16, 24, dummy) == -1
    assert lib.pfnl_stream_format(None, 1, 1, 1, 0) == -1 and b"NULL" in lib.pfnl_last_error()


def test_video_stream_checks_its_format_arguments_before_it_touches_the_engine():
    from pfnl_amd.stream import VideoStream, format_arguments, frame_shapes
    assert format_arguments() == (0, 0, 1, 0)
    assert format_arguments("nv12") == (1, 1, 1, 0)
    assert format_arguments("nv12", "rgb24", "bt601", True) == (1, 0, 0, 1)
    assert format_arguments("rgb24", "i420") == (0, 2, 1, 0)
    for kw in ({"pixel_format": "yuv420p"}, {"out_format": "NV12"}, {"matrix": "bt2020"}, {"full_range": 2}, {"pixel_format": None}):
        with pytest.raises(ValueError):
            format_arguments(**kw)
        with pytest.raises(ValueError):                                         # no engine is needed to hear about it
            VideoStream(None, 16, 24, 1, None, **kw)
    assert frame_shapes("rgb24", 16, 24) == ((16, 24, 3),)
    assert frame_shapes("nv12", 16, 24) == frame_shapes("i420", 16, 24) == ((24, 24), (576,))
