"""Chroma siting, the device-free side (include/pfnl_hip.h SITING; pfnl_amd/yuv.py, pfnl_amd/depth10.py): the rule's known answers, what it
preserves, that "left" is the rule as it was, the rule against a brute force written from the sample POSITIONS in exact rationals, and the
refusals of the new C-ABI entries and of ``siting_arguments``."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from pfnl_amd import _capi, depth10, yuv
from pfnl_amd.stream import siting_arguments

SHAPES_LEFT = [(2, 2), (2, 6), (6, 2), (18, 34), (16, 64)]
SHAPES_BRUTE = [(2, 2), (2, 6), (6, 2), (6, 10)]
# chroma sample (j, i) sits at the luma coordinates (2 j + OFF[siting][0], 2 i + OFF[siting][1])
OFF = {"left": (Fraction(1, 2), Fraction(0)), "center": (Fraction(1, 2), Fraction(1, 2)), "topleft": (Fraction(0), Fraction(0))}
SITED = ["pfnl_op_yuv420_to_rgb_u8_sited", "pfnl_op_yuv420_to_rgb_u8_surface_sited", "pfnl_op_rgb_to_yuv420_u8_sited",
         "pfnl_op_rgb_to_yuv420_u10_sited", "pfnl_stream_chroma_siting"]


def test_the_three_sitings_and_their_axes():
    assert yuv.SITINGS == ("left", "center", "topleft")
    assert yuv.AXES == {"left": (True, False), "center": (True, True), "topleft": (False, False)}
    assert [_capi.CHROMA_SITINGS[s] for s in yuv.SITINGS] == [0, 1, 2] and [yuv.siting_id(s) for s in yuv.SITINGS] == [0, 1, 2]
    for bad in ("centre", "top", None, 1):
        with pytest.raises(ValueError):
            yuv.upsample(np.zeros((1, 1)), 2, 2, bad)
        with pytest.raises(ValueError):
            yuv.downsample(np.zeros((2, 2), np.int32), bad)


# ---- the known answers, H x W = 8 x 16 ----------------------------------------------------------------------------------------------------
def test_known_answers_decode():
    H, W = 8, 16
    ramp_x = np.tile(8 * np.arange(W // 2), (H // 2, 1))
    ramp_y = np.tile(8 * np.arange(H // 2)[:, None], (1, W // 2))
    want_x = {"left": [8, 12, 16, 20, 24, 28], "center": [6, 10, 14, 18, 22, 26], "topleft": [8, 12, 16, 20, 24, 28]}
    want_y = {"left": [6, 10, 14, 18], "center": [6, 10, 14, 18], "topleft": [8, 12, 16, 20]}
    for s in yuv.SITINGS:
        assert list(yuv.upsample(ramp_x, H, W, s)[3, 2:8]) == want_x[s], s
        assert list(yuv.upsample(ramp_y, H, W, s)[2:6, 5]) == want_y[s], s


def test_known_answers_encode():
    H, W = 8, 16
    num_x = np.tile((4 * np.arange(W)) << yuv.F, (H, 1))
    num_y = np.tile(((4 * np.arange(H)) << yuv.F)[:, None], (1, W))
    want_x = {"left": [8, 16, 24, 32], "center": [10, 18, 26, 34], "topleft": [8, 16, 24, 32]}
    want_y = {"left": [10, 18], "center": [10, 18], "topleft": [8, 16]}
    for s in yuv.SITINGS:
        assert list(yuv.downsample(num_x, s)[0, 1:5].astype(int) - 128) == want_x[s], s
        assert list(yuv.downsample(num_y, s)[1:3, 0].astype(int) - 128) == want_y[s], s
        assert list(depth10.downsample10(num_x, s)[0, 1:5].astype(int) - 512) == want_x[s], s
        assert list(depth10.downsample10(num_y, s)[1:3, 0].astype(int) - 512) == want_y[s], s


@pytest.mark.parametrize("siting", yuv.SITINGS)
def test_constants_are_preserved_in_both_directions(siting):
    for H, W in SHAPES_BRUTE + [(8, 16)]:
        for v in (0, 1, 77, 128, 254, 255):
            assert (yuv.upsample(np.full((H // 2, W // 2), v), H, W, siting) == v).all()
        for v in (-128, -1, 0, 1, 50, 127):                              # a constant numerator v << F encodes to offset + v
            assert (yuv.downsample(np.full((H, W), v << yuv.F, np.int32), siting) == 128 + v).all()
        for v in (-512, -3, 0, 7, 511):
            assert (depth10.downsample10(np.full((H, W), v << yuv.F), siting) == 512 + v).all()


# ---- "left" is the rule as it was ---------------------------------------------------------------------------------------------------------
def _upsample_as_it_was(C_, H, W):
    """pfnl_amd/yuv.py upsample before the sitings: 3 : 1 down the rows, 1 : 1 on odd columns, >> 3"""
    C_ = np.asarray(C_).astype(np.int32)
    y, x = np.arange(H), np.arange(W)
    j, i = y >> 1, x >> 1
    jn = np.clip(np.where(y & 1, j + 1, j - 1), 0, H // 2 - 1)
    ir = np.clip(i + 1, 0, W // 2 - 1)
    near, far = C_[j], C_[jn]
    even = (6 * near[:, i] + 2 * far[:, i] + 4) >> 3
    odd = (3 * near[:, i] + far[:, i] + 3 * near[:, ir] + far[:, ir] + 4) >> 3
    return np.where((x & 1)[None, :], odd, even)


def _downsample_as_it_was(N, offset, top):
    N = np.asarray(N, np.int64)
    W = N.shape[1]
    v = N[0::2] + N[1::2]
    c = np.arange(0, W, 2)
    s = v[:, np.clip(c - 1, 0, W - 1)] + 2 * v[:, c] + v[:, np.clip(c + 1, 0, W - 1)]
    return np.clip(offset + ((s + (1 << (yuv.F + 2))) >> (yuv.F + 3)), 0, top)


@pytest.mark.parametrize("H,W", SHAPES_LEFT)
def test_left_equals_the_calls_without_a_siting(H, W):
    rng = np.random.default_rng(H * 100 + W)
    for _ in range(4):
        c = rng.integers(0, 256, (H // 2, W // 2))
        assert np.array_equal(yuv.upsample(c, H, W), _upsample_as_it_was(c, H, W))
        assert np.array_equal(yuv.upsample(c, H, W, "left"), yuv.upsample(c, H, W))
        num = rng.integers(-128 << yuv.F, 128 << yuv.F, (H, W)).astype(np.int32)
        assert np.array_equal(yuv.downsample(num), _downsample_as_it_was(num, 128, 255))
        assert np.array_equal(yuv.downsample(num, "left"), yuv.downsample(num))
        num10 = rng.integers(-512 << yuv.F, 512 << yuv.F, (H, W))
        assert np.array_equal(depth10.downsample10(num10), _downsample_as_it_was(num10, 512, 1023))
        assert np.array_equal(depth10.downsample10(num10, "left"), depth10.downsample10(num10))
        frame = rng.integers(0, 256, (H * 3 // 2, W), dtype=np.uint8)
        rgb = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        rgb10 = rng.integers(0, 1024, (H, W, 3)).astype(np.uint16)
        for fmt in yuv.FORMATS:
            assert np.array_equal(yuv.to_rgb(frame, fmt, H, W, "bt601", True, siting="left"), yuv.to_rgb(frame, fmt, H, W, "bt601", True))
            assert np.array_equal(yuv.from_rgb(rgb, fmt, "bt709", False, siting="left"), yuv.from_rgb(rgb, fmt, "bt709", False))
        for fmt in depth10.FORMATS:
            assert np.array_equal(depth10.from_rgb10(rgb10, fmt, siting="left"), depth10.from_rgb10(rgb10, fmt))


# ---- the rule against the positions, in exact rationals -------------------------------------------------------------------------------------
def _bilinear_taps(pos, off, n_chroma):
    """[(index, weight)]: linear interpolation at luma coordinate ``pos`` between the two nearest chroma samples of one axis (sample j at
    2 j + off), indices clamped to the plane"""
    u = (Fraction(pos) - off) / 2                                       # in chroma samples
    j0 = u.numerator // u.denominator
    t = u - j0
    clamp = lambda j: min(max(j, 0), n_chroma - 1)                      # noqa: E731
    return [(clamp(j0), 1 - t), (clamp(j0 + 1), t)]


def _footprint_taps(j, off, n_luma):
    """[(index, weight)]: the mean of the luma axis over the chroma sample's footprint - two luma pixels wide, centred on its position
    2 j + off, a luma pixel x covering [x - 1/2, x + 1/2] - indices clamped.  Midway (off 1/2) that is the box over 2j, 2j + 1; co-sited
    (off 0) the pixel 2j and half of each neighbour: 1-2-1."""
    lo, hi = 2 * j + off - 1, 2 * j + off + 1
    taps = []
    for x in range(2 * j - 2, 2 * j + 4):
        w = min(hi, x + Fraction(1, 2)) - max(lo, x - Fraction(1, 2))
        if w > 0:
            taps.append((min(max(x, 0), n_luma - 1), w / 2))
    assert sum(w for _, w in taps) == 1
    return taps


def _round_half_up(q: Fraction) -> int:
    q = q + Fraction(1, 2)
    return q.numerator // q.denominator


@pytest.mark.parametrize("siting", yuv.SITINGS)
@pytest.mark.parametrize("H,W", SHAPES_BRUTE)
def test_decode_equals_bilinear_interpolation_at_the_positions(H, W, siting):
    rng = np.random.default_rng(H * 31 + W)
    oy, ox = OFF[siting]
    for _ in range(3):
        c = rng.integers(0, 256, (H // 2, W // 2))
        got = yuv.upsample(c, H, W, siting)
        for y in range(H):
            for x in range(W):
                v = sum(wy * wx * int(c[j, i]) for j, wy in _bilinear_taps(y, oy, H // 2) for i, wx in _bilinear_taps(x, ox, W // 2))
                assert got[y, x] == _round_half_up(v), (siting, y, x)


@pytest.mark.parametrize("siting", yuv.SITINGS)
@pytest.mark.parametrize("H,W", SHAPES_BRUTE)
def test_encode_filter_equals_the_mean_over_the_footprint(H, W, siting):
    rng = np.random.default_rng(H * 37 + W)
    oy, ox = OFF[siting]
    for _ in range(3):
        num = rng.integers(-128 << yuv.F, 128 << yuv.F, (H, W)).astype(np.int32)
        s, k = yuv.encode_filter(num, siting)
        assert k == {"left": 3, "center": 2, "topleft": 4}[siting]
        got, got10 = yuv.downsample(num, siting), depth10.downsample10(num.astype(np.int64) * 4, siting)
        for j in range(H // 2):
            for i in range(W // 2):
                v = sum(wy * wx * int(num[y, x]) for y, wy in _footprint_taps(j, oy, H) for x, wx in _footprint_taps(i, ox, W))
                assert Fraction(int(s[j, i]), 1 << k) == v, (siting, j, i)           # the filter itself, unrounded
                assert got[j, i] == min(max(128 + _round_half_up(v / (1 << yuv.F)), 0), 255)
                assert got10[j, i] == min(max(512 + _round_half_up(4 * v / (1 << yuv.F)), 0), 1023)


@pytest.mark.parametrize("siting", yuv.SITINGS)
def test_greys_have_no_chroma(siting):
    rng = np.random.default_rng(7)
    for H, W in [(2, 2), (6, 10)]:
        grey = np.repeat(rng.integers(0, 256, (H, W, 1), dtype=np.uint8), 3, axis=2)
        grey10 = np.repeat(rng.integers(0, 1024, (H, W, 1)).astype(np.uint16), 3, axis=2)
        for matrix in ("bt601", "bt709"):
            for full in (False, True):
                _, cb, cr = yuv.planes(yuv.from_rgb(grey, "i420", matrix, full, siting=siting), "i420", H, W)
                assert (cb == 128).all() and (cr == 128).all()
                _, cb, cr = depth10.planes10(depth10.from_rgb10(grey10, "p010", matrix, full, siting=siting), "p010", H, W)
                assert (cb == 512).all() and (cr == 512).all()


# ---- the C-ABI and the keywords, without a device ---------------------------------------------------------------------------------------------
def test_sited_entries_are_declared_and_refuse_without_a_device():
    assert set(SITED) <= set(_capi.SIGNATURES)
    lib = _capi.load_library()
    assert lib.pfnl_version() == 4                                       # symbols were added, nothing changed
    dummy = C.c_void_p(16)                                               # never dereferenced: the calls return first
    sf = _capi.pfnl_surface()
    for k in range(3):
        sf.plane[k], sf.pitch[k] = 4096, 64
    for bad in (-1, 3, 7):
        assert lib.pfnl_op_yuv420_to_rgb_u8_sited(dummy, 1, 1, 0, 1, 4, 4, dummy, bad, None) == -1 and b"siting" in lib.pfnl_last_error()
        assert lib.pfnl_op_yuv420_to_rgb_u8_surface_sited(C.byref(sf), 2, 1, 0, 4, 4, dummy, bad, None) == -1 and b"siting" in lib.pfnl_last_error()
        assert lib.pfnl_op_rgb_to_yuv420_u8_sited(dummy, 2, 0, 1, 1, 4, 4, dummy, bad, None) == -1 and b"siting" in lib.pfnl_last_error()
        assert lib.pfnl_op_rgb_to_yuv420_u10_sited(dummy, 4, 0, 1, 1, 4, 4, dummy, bad, None) == -1 and b"siting" in lib.pfnl_last_error()
        assert lib.pfnl_stream_chroma_siting(dummy, bad, 0) == -1 and b"siting" in lib.pfnl_last_error()
        assert lib.pfnl_stream_chroma_siting(dummy, 0, bad) == -1 and b"siting" in lib.pfnl_last_error()
    assert lib.pfnl_stream_chroma_siting(None, 0, 0) == -1 and b"NULL" in lib.pfnl_last_error()
    # the arguments the plain hooks refuse are refused here as well, with a good siting
    assert lib.pfnl_op_yuv420_to_rgb_u8_sited(None, 1, 1, 0, 1, 4, 4, dummy, 1, None) == -1 and b"NULL" in lib.pfnl_last_error()
    assert lib.pfnl_op_rgb_to_yuv420_u8_sited(dummy, 0, 1, 0, 1, 4, 4, dummy, 1, None) == -1 and b"fmt" in lib.pfnl_last_error()
    assert lib.pfnl_op_rgb_to_yuv420_u10_sited(dummy, 4, 0, 1, 1, 4, 3, dummy, 2, None) == -1 and b"even" in lib.pfnl_last_error()


def test_siting_arguments():
    assert siting_arguments() == (0, 0)
    assert siting_arguments("center") == (1, 1)
    assert siting_arguments("center", "left") == (1, 0)
    assert siting_arguments("left", "topleft") == (0, 2)
    for bad in [("centre", None), ("left", "top"), (1, None), (None, None), ("left", 2), (["left"], None)]:
        with pytest.raises(ValueError):
            siting_arguments(*bad)
