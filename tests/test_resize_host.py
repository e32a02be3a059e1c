"""The resampling rule of the streaming session's output size (pfnl_amd/resize.py; include/pfnl_hip.h pfnl_stream_resize), without a device:
the properties the kernel's integer widths rest on, the library's 128-bit tables against the numpy statement, the limits, and a sanity
comparison with Pillow's BICUBIC in the interior."""
import ctypes as C
import math

import numpy as np
import pytest

from pfnl_amd import _capi, resize

I32P, I16P = C.POINTER(C.c_int32), C.POINTER(C.c_int16)
INTERIOR_2_TO_1 = [-192, -576, 1856, 7104, 7104, 1856, -576, -192]


def _ratios(n_in):
    """about 37 sizes from a quarter of n_in up to n_in, and three enlargements"""
    outs = {int(v) for v in np.linspace((n_in + 3) // 4, n_in, 37)}
    return sorted(outs | {n_in + 1, 3 * n_in // 2, 2 * n_in})


@pytest.mark.parametrize("n_in", [64, 100, 1080, 2160])
def test_rows_sum_to_one_stay_inside_int16_and_are_contiguous(n_in):
    worst = 0
    for n_out in _ratios(n_in):
        first, count, coef = resize.taps(n_in, n_out)
        assert first.shape == count.shape == (n_out,) and coef.shape == (n_out, count.max())
        assert (coef.sum(axis=1) == 1 << 14).all(), (n_in, n_out)
        mag = np.abs(coef).sum(axis=1)
        assert (mag <= 1 << 15).all(), (n_in, n_out, int(mag.max()))
        worst = max(worst, int(mag.max()))
        # one run per row, inside the input, zero behind it; neither end ever moves back (the kernel sizes its tile by that)
        assert (count >= 1).all() and (first >= 0).all() and (first + count <= n_in).all()
        assert (coef[np.arange(coef.shape[1])[None, :] >= count[:, None]] == 0).all()
        assert (np.diff(first) >= 0).all() and (np.diff(first + count) >= 0).all()
        assert resize.max_taps(n_in, n_out) == coef.shape[1]
    assert worst <= 20788                                                        # what these ratios were seen to reach: far inside 2^15


def test_contiguity_follows_from_the_definition():
    """every index of the run carries a tap: the unclamped taps of o are consecutive integers and the clamp is monotonic"""
    for n_in, n_out in [(64, 17), (100, 101), (96, 54), (8, 2), (30, 60)]:
        d = 2 * max(n_in, n_out)
        first, count, _ = resize.taps(n_in, n_out)
        for o in range(n_out):
            js = [j for j in range(-40, n_in + 40) if abs(n_out * (2 * j + 1) - n_in * (2 * o + 1)) < 2 * d]
            assert js == list(range(js[0], js[-1] + 1))
            hit = sorted({min(max(j, 0), n_in - 1) for j in js})
            assert hit == list(range(first[o], first[o] + count[o]))


def test_two_to_one_interior_row():
    for n_out in (16, 50):
        first, count, coef = resize.taps(2 * n_out, n_out)
        for o in (3, n_out // 2, n_out - 4):
            assert count[o] == 8 and first[o] == 2 * o - 3
            assert list(coef[o]) == INTERIOR_2_TO_1
    first, count, coef = resize.taps(16, 8)                                      # at the border the clamped taps fold onto sample 0
    assert first[0] == 0 and count[0] == 5 and list(coef[0][:5]) == [-192 - 576 + 1856 + 7104, 7104, 1856, -576, -192]


def test_same_size_is_the_identity():
    rng = np.random.default_rng(1)
    for H, W in [(1, 1), (5, 7), (16, 24)]:
        x = rng.integers(0, 256, (H, W, 3), np.uint8)
        assert np.array_equal(resize.resize(x, H, W), x)


def test_constant_frames_stay_constant():
    for value in (0, 1, 77, 128, 254, 255):
        x = np.full((20, 28, 3), value, np.uint8)
        for oH, oW in [(5, 7), (7, 9), (13, 28), (20, 27), (21, 29), (30, 42), (40, 56), (11, 50)]:
            y = resize.resize(x, oH, oW)
            assert y.shape == (oH, oW, 3) and (y == value).all(), (value, oH, oW)


def test_intermediate_of_extreme_content_stays_inside_int16():
    rng = np.random.default_rng(2)
    worst = 0
    for W, oW in [(64, 16), (64, 17), (96, 54), (64, 96), (100, 101), (80, 31)]:
        small = rng.integers(0, 2, (6, (W + 1) // 2, 3), np.uint8) * 255
        x = np.repeat(np.repeat(small, 2, axis=0), 2, axis=1)[:, :W]
        h = (resize._apply(x, resize.taps(W, oW), 1) + 128) >> 8
        worst = max(worst, int(np.abs(h).max()))
    assert worst <= 255 * (1 << 15) // 256 + 1 < 1 << 15                         # the bound sum |c| <= 2^15 gives; seen: about 18 000


def _c_taps(lib, n_in, n_out):
    nt = C.c_int(0)
    assert lib.pfnl_resize_max_taps(n_in, n_out, C.byref(nt)) == 0, lib.pfnl_last_error()
    first, count = np.full(n_out, -7, np.int32), np.full(n_out, -7, np.int32)
    coef = np.full((n_out, nt.value), 77, np.int16)                              # (the padding must come back as zeros)
    assert lib.pfnl_resize_taps(n_in, n_out, first.ctypes.data_as(I32P), count.ctypes.data_as(I32P), coef.ctypes.data_as(I16P)) == 0
    return first, count, coef


@pytest.mark.parametrize("n_in,n_out", [(8, 2), (64, 16), (64, 17), (96, 54), (64, 128), (100, 101), (2160, 1080), (4320, 2161), (7680, 3841),
                                        (1080, 2160)])
def test_library_tables_equal_the_numpy_rule(n_in, n_out):
    lib = _capi.load_library()
    first, count, coef = _c_taps(lib, n_in, n_out)
    want = resize.taps(n_in, n_out)
    assert coef.shape == want[2].shape
    assert np.array_equal(first, want[0]) and np.array_equal(count, want[1]) and np.array_equal(coef, want[2])


def test_limits_and_null_arguments_are_refused_without_a_device():
    lib = _capi.load_library()
    nt = C.c_int(-5)
    a, b = np.zeros(64, np.int32), np.zeros((64, 32), np.int16)
    pa, pb = a.ctypes.data_as(I32P), b.ctypes.data_as(I16P)
    for n_in, n_out in [(64, 15), (64, 129), (65, 16), (0, 4), (4, 0), (-8, 8), (16385, 16384), (16384, 16385), (8193, 16386)]:
        assert lib.pfnl_resize_max_taps(n_in, n_out, C.byref(nt)) == -1 and b"resize" in lib.pfnl_last_error(), (n_in, n_out)
        assert lib.pfnl_resize_taps(n_in, n_out, pa, pa, pb) == -1
        with pytest.raises(ValueError):
            resize.check_limits(n_in, n_out)
    assert nt.value == -5
    for n_in, n_out in [(64, 16), (65, 17), (64, 128), (16384, 4096), (1, 1), (1, 2)]:     # the limits themselves are inside
        assert lib.pfnl_resize_max_taps(n_in, n_out, C.byref(nt)) == 0, (n_in, n_out)
        resize.check_limits(n_in, n_out)
    assert lib.pfnl_resize_max_taps(8, 8, None) == -1 and b"NULL" in lib.pfnl_last_error()
    assert lib.pfnl_resize_taps(8, 8, None, pa, pb) == -1 and lib.pfnl_resize_taps(8, 8, pa, None, pb) == -1
    assert lib.pfnl_resize_taps(8, 8, pa, pa, None) == -1
    dummy = C.c_void_p(16)                                                       # never dereferenced: the hooks return first
    assert lib.pfnl_op_resize_u8(None, 1, 8, 8, 8, 8, dummy, None) == -1 and b"NULL" in lib.pfnl_last_error()
    assert lib.pfnl_op_resize_u8(dummy, 1, 8, 8, 8, 8, None, None) == -1
    assert lib.pfnl_op_resize_u8(dummy, 0, 8, 8, 8, 8, dummy, None) == -1
    assert lib.pfnl_op_resize_u8(dummy, 1, 8, 8, 1, 8, dummy, None) == -1 and b"quarter" in lib.pfnl_last_error()
    assert lib.pfnl_op_resize_u8(dummy, 1, 8, 8, 8, 17, dummy, None) == -1
    assert lib.pfnl_op_resize_u8(dummy, 1, 8, 20000, 8, 16000, dummy, None) == -1
    assert lib.pfnl_stream_resize(None, 8, 8) == -1 and b"NULL" in lib.pfnl_last_error()


def test_stream_arguments_without_a_device():
    from pfnl_amd.stream import resize_arguments
    assert resize_arguments(None, 64, 96) == (0, 0)
    assert resize_arguments((36, 54), 64, 96) == (36, 54) and resize_arguments([37, 55], 64, 96, "rgb24") == (37, 55)
    assert resize_arguments((36, 54), 64, 96, "nv12") == (36, 54)
    for bad, fmt in [((15, 54), "rgb24"), ((36, 193), "rgb24"), ((37, 54), "nv12"), ((36, 55), "i420"), (36, "rgb24"), ((1, 2, 3), "rgb24"),
                     ("ab", "rgb24")]:
        with pytest.raises(ValueError):
            resize_arguments(bad, 64, 96, fmt)


@pytest.mark.parametrize("size,out", [((64, 96), (16, 24)), ((64, 96), (17, 25)), ((64, 96), (36, 54)), ((64, 96), (45, 77)),
                                      ((64, 96), (128, 192)), ((64, 96), (90, 100)), ((72, 120), (54, 90))])
def test_interior_agrees_with_pillow_bicubic(size, out):
    """A sanity check against an independent implementation of the same filter, not the rule's definition: Pillow works in 8-bit passes with
    its own coefficient precision, and at the borders it drops the taps outside the frame where this rule clamps."""
    Image = pytest.importorskip("PIL.Image")
    (H, W), (oH, oW) = size, out
    y, x = np.mgrid[0:H, 0:W]
    frame = np.stack([np.round(127 + 120 * np.sin(x / 5 + y / 7 + c)) for c in range(3)], axis=-1).astype(np.uint8)
    bicubic = getattr(Image, "Resampling", Image).BICUBIC
    want = np.asarray(Image.fromarray(frame).resize((oW, oH), bicubic)).astype(np.int32)
    got = resize.resize(frame, oH, oW).astype(np.int32)
    my = math.ceil(2 * max(1, H / oH) * oH / H) + 1
    mx = math.ceil(2 * max(1, W / oW) * oW / W) + 1
    delta = np.abs(got - want)[my:oH - my, mx:oW - mx]
    assert delta.size > 0
    print(size, out, "max |delta| interior", int(delta.max()))
    assert delta.max() <= 1, (size, out, int(delta.max()))
