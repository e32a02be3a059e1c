"""10-bit input without a device: the host rule the 16-bit input edge is tested against (pfnl_amd/depth10.py decode_coefficients10, values10,
to_rgb10, dequantise10; pfnl_amd/scene.py luma_u10, frame_sad10), C420p10 in pfnl_amd/y4m.py, the in_depth keyword of open_stream and of
pfnl_amd.upscale, and the arguments the new C-ABI entries refuse before any HIP call."""
import ctypes as C
import io

import numpy as np
import pytest

from pfnl_amd import _capi, depth10, scene, stream, upscale as up, y4m, yuv

PAIRS = [("bt601", False), ("bt709", False), ("bt601", True), ("bt709", True)]
DOCUMENTED = {("bt601", False): (19133, 26226, -6438, -13359, 33148), ("bt709", False): (19133, 29459, -3504, -8757, 34711),
              ("bt601", True): (16384, 22970, -5638, -11700, 29032), ("bt709", True): (16384, 25802, -3069, -7670, 30402)}


def _const(H, W, y, cb, cr, fmt):
    return depth10.pack10(np.full((H, W), y), np.full((H // 2, W // 2), cb), np.full((H // 2, W // 2), cr), fmt)


# ---- coefficients --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matrix,full", PAIRS)
def test_decode_coefficients_are_the_documented_integers_and_the_librarys(matrix, full):
    y0, dec = depth10.decode_coefficients10(matrix, full)
    assert (y0, dec) == (0 if full else 64, DOCUMENTED[matrix, full])
    assert y0 == depth10.coefficients10(matrix, full)[0]
    out = (C.c_int32 * 6)()
    lib = _capi.load_library()
    assert lib.pfnl_yuv10_decode_coefficients(_capi.YUV_MATRICES[matrix], int(full), out) == 0
    assert tuple(out) == (y0,) + dec
    assert lib.pfnl_yuv10_decode_coefficients(2, 0, out) == -1 and lib.pfnl_yuv10_decode_coefficients(0, 2, out) == -1
    assert lib.pfnl_yuv10_decode_coefficients(0, 0, None) == -1 and b"NULL" in lib.pfnl_last_error()
    with pytest.raises(ValueError):
        depth10.decode_coefficients10("bt2020", full)


# ---- to_rgb10 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", depth10.FORMATS)
def test_known_answers_on_constant_frames(fmt):
    for matrix in ("bt601", "bt709"):
        for y, want in ((64, 0), (940, 1023), (502, 511)):
            rgb = depth10.to_rgb10(_const(4, 6, y, 512, 512, fmt), fmt, 4, 6, matrix, False)
            assert rgb.dtype == np.uint16 and rgb.shape == (4, 6, 3) and (rgb == want).all(), (matrix, y)
        for y in (0, 1, 511, 512, 1022, 1023):                                  # full-range greys: the identity
            assert (depth10.to_rgb10(_const(2, 2, y, 512, 512, fmt), fmt, 2, 2, matrix, True) == y).all()
        for siting in yuv.SITINGS:                                              # a constant frame does not depend on the siting
            assert (depth10.to_rgb10(_const(4, 4, 502, 512, 512, fmt), fmt, 4, 4, matrix, False, siting) == 511).all()


@pytest.mark.parametrize("matrix,full", PAIRS)
def test_to_rgb10_is_within_one_code_of_the_real_equations(matrix, full):
    """All 1024 luma values x a chroma grid, constant chroma: |integer - real| <= 1 where the real value is not clipped (the statement
    tests/test_yuv_host.py makes at 8 bits; the worst here is about 0.54)."""
    kr, kb = depth10.MATRICES[matrix]
    kg = 1.0 - kr - kb
    y0, ys, cs = (0.0, 1.0, 1.0) if full else (64.0, 876.0 / 1023.0, 896.0 / 1023.0)
    grid = sorted(set(list(range(0, 1024, 73)) + [64, 511, 512, 513, 960, 1023]))
    Y = np.tile(np.arange(1024, dtype=np.uint16).reshape(2, 512), (1, 1))       # one frame of 2 x 512 holds every luma value
    worst = 0.0
    for cb in grid:
        for cr in grid:
            frame = depth10.pack10(Y, np.full((1, 256), cb), np.full((1, 256), cr), "i010")
            got = depth10.to_rgb10(frame, "i010", 2, 512, matrix, full).astype(np.float64)
            yy, u, v = (Y.astype(np.float64) - y0) / ys, (cb - 512.0) / cs, (cr - 512.0) / cs
            real = np.stack([yy + 2 * (1 - kr) * v, yy - 2 * kb * (1 - kb) / kg * u - 2 * kr * (1 - kr) / kg * v, yy + 2 * (1 - kb) * u], -1)
            inside = (real >= 0) & (real <= 1023)
            worst = max(worst, float(np.abs(got - real)[inside].max()))
            assert np.array_equal(got[real < -1], np.zeros_like(got)[real < -1]) and (got[real > 1024] == 1023).all()
    print(f"{matrix} full={full}: worst unclipped |integer - real| = {worst:.3f}")
    assert worst <= 1.0


def test_values10_is_lenient_where_planes10_is_strict():
    rng = np.random.default_rng(3)
    H, W = 6, 8
    clean = depth10.pack10(rng.integers(0, 1024, (H, W)), rng.integers(0, 1024, (H // 2, W // 2)), rng.integers(0, 1024, (H // 2, W // 2)), "p010")
    dirty = clean | rng.integers(0, 64, clean.shape).astype(np.uint16)
    assert (dirty != clean).any()
    with pytest.raises(ValueError):
        depth10.planes10(dirty, "p010", H, W)
    assert np.array_equal(depth10.values10(dirty, "p010"), clean >> 6) and int(depth10.values10(dirty, "p010").max()) <= 1023
    for matrix, full in PAIRS:
        assert np.array_equal(depth10.to_rgb10(dirty, "p010", H, W, matrix, full), depth10.to_rgb10(clean, "p010", H, W, matrix, full))
    i010 = depth10.pack10(*depth10.planes10(clean, "p010", H, W), "i010")
    high = i010.copy()
    where = rng.random(high.shape) < 0.2
    high[where] = rng.integers(1024, 65536, int(where.sum())).astype(np.uint16)
    assert np.array_equal(depth10.values10(high, "i010"), np.where(where, 1023, i010))
    assert np.array_equal(depth10.values10(high, "rgb10"), np.where(where, 1023, i010))
    with pytest.raises(ValueError):
        depth10.planes10(high, "i010", H, W)
    topped = np.where(where, 1023, i010).astype(np.uint16)
    assert np.array_equal(depth10.to_rgb10(high, "i010", H, W), depth10.to_rgb10(topped, "i010", H, W))
    with pytest.raises(ValueError):
        depth10.values10(high, "nv12")
    with pytest.raises(ValueError):
        depth10.values10(high.astype(np.int32), "i010")
    with pytest.raises(ValueError):
        depth10.to_rgb10(high[:-1], "i010", H, W)


def test_to_rgb10_numerators_fit_int32_over_the_whole_cube():
    worst = 0
    for matrix, full in PAIRS:
        y0, (dy, drv, dgu, dgv, dbu) = depth10.decode_coefficients10(matrix, full)
        for y in (0, 1023):
            for u in (-512, 511):
                for v in (-512, 511):
                    yy = dy * (y - y0)
                    worst = max(worst, *(abs(n) for n in (yy + drv * v, yy + dgu * u + dgv * v, yy + dbu * u)))
    assert worst == 36085868 and worst + (1 << 13) < (1 << 31)                  # (ahead of the rounding term)


# ---- dequantise10 --------------------------------------------------------------------------------------------------------------------------
def test_dequantise10_is_the_double_division_rounded_once():
    v = np.arange(1024, dtype=np.uint16)
    d = depth10.dequantise10(v)
    assert d.dtype == np.float32 and d[0] == 0.0 and d[1023] == 1.0 and (np.diff(d) > 0).all()
    for i in range(1024):
        assert d[i] == np.float32(i / 1023.0)                                   # Python's division is the double one
    differ = int((d != v.astype(np.float32) * np.float32(1.0 / 1023.0)).sum())
    print(f"dequantise10: {differ} of 1024 values differ from v * float32(1 / 1023)")   # the reason for a table on the device
    assert np.array_equal(depth10.dequantise10(np.array([1024, 4095, 65535], np.uint16)), np.ones(3, np.float32))
    assert depth10.dequantise10(np.zeros((2, 3, 3), np.uint16)).shape == (2, 3, 3)
    with pytest.raises(ValueError):
        depth10.dequantise10(np.zeros(4, np.uint8))


# ---- scenes --------------------------------------------------------------------------------------------------------------------------------
def test_luma_u10_and_frame_sad10_against_python_integers():
    rng = np.random.default_rng(5)
    for H, W in ((1, 1), (3, 5), (4, 8)):
        a, b = (rng.integers(0, 1024, (H, W, 3)).astype(np.uint16) for _ in range(2))
        a[0, 0, 0] = 40000                                                      # above 1023: counts as 1023
        la = scene.luma_u10(a)
        total = 0
        for y in range(H):
            for x in range(W):
                ya = (66 * min(int(a[y, x, 0]), 1023) + 129 * int(a[y, x, 1]) + 25 * int(a[y, x, 2]) + 512) >> 10
                yb = (66 * int(b[y, x, 0]) + 129 * int(b[y, x, 1]) + 25 * int(b[y, x, 2]) + 512) >> 10
                assert la[y, x] == ya
                total += abs(ya - yb)
        assert scene.frame_sad10(a, b) == total == scene.frame_sad10(b, a)
        assert scene.frame_sads10([a, b, b]) == [0, total, 0]
    assert int(scene.luma_u10(np.full((1, 1, 3), 1023, np.uint16))[0, 0]) == 220   # white on the 8-bit scale: (220 * 1023 + 512) >> 10
    with pytest.raises(ValueError):
        scene.luma_u10(np.zeros((2, 2, 3), np.uint8))


def test_luma_u10_keeps_the_8_bit_scale():
    """An 8-bit frame widened by bit replication, (v << 2) | (v >> 6): its 10-bit luma is within 1 of luma_u8, so a threshold means the same."""
    rng = np.random.default_rng(7)
    f8 = rng.integers(0, 256, (64, 64, 3)).astype(np.uint8)
    f8[0, :4] = [[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 255]]
    f10 = ((f8.astype(np.uint16) << 2) | (f8 >> 6)).astype(np.uint16)
    diff = np.abs(scene.luma_u10(f10) - scene.luma_u8(f8))
    assert int(diff.max()) == 1
    g8 = rng.integers(0, 256, f8.shape).astype(np.uint8)
    g10 = ((g8.astype(np.uint16) << 2) | (g8 >> 6)).astype(np.uint16)
    assert abs(scene.frame_sad10(f10, g10) - scene.frame_sad(f8, g8)) <= 2 * 64 * 64


def test_scene_first_takes_a_depth():
    rng = np.random.default_rng(9)
    dark = [rng.integers(0, 100, (8, 8, 3)).astype(np.uint16) for _ in range(3)]
    bright = [rng.integers(900, 1024, (8, 8, 3)).astype(np.uint16) for _ in range(3)]
    frames = dark + bright + dark[:2]
    assert scene.scene_first(frames, 30.0, depth=10).tolist() == [0, 0, 0, 3, 3, 3, 6, 6]
    assert scene.scene_first(frames, None, marks=[2], depth=10).tolist() == [0, 0, 2, 2, 2, 2, 2, 2]
    with pytest.raises(ValueError):
        scene.scene_first(frames, 30.0, depth=12)
    with pytest.raises(ValueError):
        scene.scene_first(frames, 30.0)                                         # (uint16 frames at the default depth of 8)


# ---- Y4M -----------------------------------------------------------------------------------------------------------------------------------
HEAD10 = b"YUV4MPEG2 W24 H16 F25:1 Ip A1:1 C420p10 XYSCSS=420P10\n"


def _frame10(H, W, k):
    return np.random.default_rng(100 + k).integers(0, 1024, (H * 3 // 2, W)).astype(np.uint16)


def _stream10(head, frames):
    return head + b"".join(b"FRAME\n" + f.astype("<u2").tobytes() for f in frames)


def test_y4m_reads_c420p10_where_asked():
    h = y4m.Y4MHeader.parse(HEAD10, depths=(8, 10))
    assert (h.width, h.height, h.bits, h.siting, h.frame_bytes) == (24, 16, 10, "left", 24 * 16 * 3)
    assert y4m.Y4MHeader.parse(HEAD10.replace(b"C420p10", b"C420mpeg2"), depths=(8, 10)).bits == 8
    for refuse in (lambda: y4m.Y4MHeader.parse(HEAD10), lambda: y4m.Y4MReader(io.BytesIO(HEAD10)), lambda: y4m.Y4MHeader.parse(HEAD10, depths=(8,))):
        with pytest.raises(ValueError, match="C420p10"):
            refuse()
    frames = [_frame10(16, 24, k) for k in range(3)]
    data = _stream10(HEAD10, frames)
    r = y4m.Y4MReader(io.BytesIO(data), depths=(8, 10))
    got = list(r)
    assert r.frames == 3 and all(g.dtype == np.dtype("<u2") and g.shape == (24, 24) and np.array_equal(g, f) for g, f in zip(got, frames))
    out = io.BytesIO()
    w = y4m.Y4MWriter(out, r.header)
    for g in got:
        w.write_frame(g)
    assert out.getvalue() == data                                               # byte for byte
    with pytest.raises(ValueError, match="frame 2 is truncated"):
        list(y4m.Y4MReader(io.BytesIO(data[:-5]), depths=(8, 10)))


# ---- open_stream and the library, before any device ---------------------------------------------------------------------------------------
def test_in_depth_is_checked_before_the_engine_is_touched():
    for bad in (12, 16, 0, "10", None, 10.5, True):
        with pytest.raises(ValueError, match="in_depth"):
            stream.VideoStream(None, 16, 24, 1, in_depth=bad)
        with pytest.raises(ValueError, match="in_depth"):
            stream.depth_argument(bad)
    assert stream.depth_argument() == 8 and stream.depth_argument(10) == 10
    assert [stream.pushed_format(f, 10) for f in ("rgb24", "nv12", "i420")] == ["rgb10", "p010", "i010"]
    assert [stream.pushed_format(f, 8) for f in ("rgb24", "nv12", "i420")] == ["rgb24", "nv12", "i420"]
    ok = stream.frame_argument(np.zeros((24, 24), np.uint16), "i420", 16, 24, 10)
    assert ok.dtype == np.uint16 and ok.flags.c_contiguous
    assert stream.frame_argument(np.zeros((16, 24, 3), np.uint16), "rgb24", 16, 24, 10).shape == (16, 24, 3)
    assert stream.frame_argument(np.zeros(16 * 24 * 3 // 2, np.uint16), "nv12", 16, 24, 10).shape == (576,)
    for frame, fmt, depth in ((np.zeros((24, 24), np.uint8), "i420", 10), (np.zeros((24, 24), np.uint16), "i420", 8),
                              (np.zeros((24, 22), np.uint16), "i420", 10), (np.zeros((16, 24, 3), np.int16), "rgb24", 10),
                              (np.zeros((16, 24), np.uint16), "rgb24", 10)):
        with pytest.raises(ValueError, match="expected a uint"):
            stream.frame_argument(frame, fmt, 16, 24, depth)


def test_the_new_entries_refuse_bad_arguments_without_a_device():
    lib = _capi.load_library()
    d = C.c_void_p(64)                                                          # never dereferenced: the entries return first
    assert lib.pfnl_stream_input_depth(None, 10) == -1 and b"NULL" in lib.pfnl_last_error()
    dec = lambda yuv, fmt, m, fr, n, H, W, rgb, sit: lib.pfnl_op_yuv420_to_rgb_u10_sited(yuv, fmt, m, fr, n, H, W, rgb, sit, None)   # noqa: E731
    assert dec(None, 4, 1, 0, 1, 4, 4, d, 0) == -1 and b"NULL" in lib.pfnl_last_error()
    assert dec(d, 4, 1, 0, 1, 4, 4, None, 0) == -1 and b"NULL" in lib.pfnl_last_error()
    for fmt in (0, 1, 2, 3, 6, -1):
        assert dec(d, fmt, 1, 0, 1, 4, 4, d, 0) == -1 and b"P010" in lib.pfnl_last_error()
    assert dec(d, 4, 2, 0, 1, 4, 4, d, 0) == -1 and dec(d, 5, 1, 2, 1, 4, 4, d, 0) == -1
    for n, H, W in ((0, 4, 4), (1, 3, 4), (1, 4, 5), (1, 0, 4), (1, 4, -2)):
        assert dec(d, 5, 1, 0, n, H, W, d, 0) == -1 and b"even" in lib.pfnl_last_error()
    assert dec(d, 5, 1, 0, 1, 4, 4, d, 3) == -1 and b"siting" in lib.pfnl_last_error()
    assert dec(C.c_void_p(65), 5, 1, 0, 1, 4, 4, d, 0) == -1 and b"2-byte" in lib.pfnl_last_error()
    sf = _capi.pfnl_surface((C.c_void_p * 3)(64, 128, None), (C.c_size_t * 3)(8, 8, 0))
    surf = lambda s, fmt, H, W, rgb: lib.pfnl_op_yuv420_to_rgb_u10_surface_sited(s, fmt, 1, 0, H, W, rgb, 0, None)   # noqa: E731
    assert surf(None, 4, 4, 4, d) == -1 and b"NULL" in lib.pfnl_last_error()
    assert surf(C.byref(sf), 1, 4, 4, d) == -1 and b"P010" in lib.pfnl_last_error()
    assert surf(C.byref(sf), 4, 4, 3, d) == -1 and b"even" in lib.pfnl_last_error()
    assert surf(C.byref(sf), 5, 4, 4, d) == -1 and b"plane" in lib.pfnl_last_error()       # I010 has three planes
    assert surf(C.byref(sf), 4, 4, 6, d) == -1 and b"pitch" in lib.pfnl_last_error()       # rows of 12 bytes in a pitch of 8
    odd = _capi.pfnl_surface((C.c_void_p * 3)(64, 128, None), (C.c_size_t * 3)(9, 8, 0))
    assert surf(C.byref(odd), 4, 4, 4, d) == -1 and b"even" in lib.pfnl_last_error()
    g = lambda ring, win, cap, last, first, count, T, H, W: lib.pfnl_op_gather_windows_u10(ring, win, cap, last, first, count, T, H, W, None)   # noqa: E731
    assert g(None, d, 5, 4, 0, 1, 5, 2, 2) == -1 and b"NULL" in lib.pfnl_last_error()
    assert g(d, d, 5, 4, 0, 1, 4, 2, 2) == -1 and b"geometry" in lib.pfnl_last_error()     # T even
    assert g(d, d, 5, 4, 0, 1, 5, 1, 1) == -1 and b"geometry" in lib.pfnl_last_error()     # H*W*3 odd
    assert g(d, d, 5, 4, 4, 2, 5, 2, 2) == -1 and b"beyond" in lib.pfnl_last_error()
    assert g(d, d, 3, 9, 2, 3, 5, 2, 2) == -1 and b"ring holds" in lib.pfnl_last_error()
    assert g(C.c_void_p(66), d, 5, 4, 0, 1, 5, 2, 2) == -1 and b"aligned" in lib.pfnl_last_error()
    assert lib.pfnl_op_gather_windows_u10_scenes(d, None, d, 5, 4, 0, 1, 5, 2, 2, None) == -1 and b"NULL" in lib.pfnl_last_error()
    assert lib.pfnl_op_gather_windows_u10_scenes(d, C.c_void_p(68), d, 5, 4, 0, 1, 5, 2, 2, None) == -1 and b"aligned" in lib.pfnl_last_error()
    assert lib.pfnl_op_scene_sad_u10(None, d, 2, 2, d, None) == -1 and b"NULL" in lib.pfnl_last_error()
    assert lib.pfnl_op_scene_sad_u10(d, d, 0, 2, d, None) == -1 and b"positive" in lib.pfnl_last_error()
    assert lib.pfnl_op_scene_sad_u10(C.c_void_p(65), d, 2, 2, d, None) == -1 and b"2-byte" in lib.pfnl_last_error()
    assert lib.pfnl_op_scene_sad_u10(d, d, 2, 2, C.c_void_p(68), None) == -1 and b"8-byte" in lib.pfnl_last_error()


# ---- pfnl_amd.upscale around a stub session ------------------------------------------------------------------------------------------------
class _Stub:
    """What upscale() needs of a session: it records its keywords and delivers each pushed frame, 4 x nearest, at the output depth."""

    def __init__(self, log, H, W, batch, **kw):
        log.append(dict(kw, H=H, W=W, batch=batch))
        self.kw, self.scale, self.out_size = kw, 4, kw.get("out_size")
        self.out_chroma_siting = kw.get("out_chroma_siting") or kw["chroma_siting"]
        self.pushed, self.closed, self.H, self.W = [], False, H, W

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.closed = True

    def _sr(self, f):
        planes = depth10.planes10(f, "i010", self.H, self.W) if f.dtype == np.uint16 else yuv.planes(f, "i420", self.H, self.W)
        big = [np.repeat(np.repeat(p, 4, 0), 4, 1) for p in planes]
        if self.kw["out_format"] == "i010":
            return depth10.pack10(*[p if f.dtype == np.uint16 else p.astype(np.uint16) << 2 for p in big], "i010")
        return yuv.pack(*[(p >> 2).astype(np.uint8) if f.dtype == np.uint16 else p for p in big], "i420")

    def push(self, frame):
        self.pushed.append(frame)
        return [(len(self.pushed) - 1, self._sr(frame))]

    def end(self):
        return []


def _run_upscale(data, **kw):
    log, made, out, err = [], [], io.BytesIO(), io.StringIO()

    def open_stream(H, W, batch=1, **k):
        made.append(_Stub(log, H, W, batch, **k))
        return made[-1]

    n = up.upscale(y4m.Y4MReader(io.BytesIO(data), depths=(8, 10)), y4m.Y4MWriter(out), open_stream, log=err, **kw)
    assert made[0].closed
    return n, log[0], out.getvalue(), made[0]


def test_upscale_opens_a_10_bit_session_for_a_10_bit_stream_only():
    frames = [_frame10(16, 24, k) for k in range(4)]
    n, kw, data, vs = _run_upscale(_stream10(HEAD10, frames), batch=2, out_format="i010")
    assert n == 4 and kw == {"H": 16, "W": 24, "batch": 2, "pixel_format": "i420", "out_format": "i010", "chroma_siting": "left",
                             "matrix": "bt601", "full_range": False, "in_depth": 10}
    assert all(f.dtype == np.uint16 and f.shape == (24, 24) and np.array_equal(f, g) for f, g in zip(vs.pushed, frames))
    head, body = data.split(b"\n", 1)
    assert head == b"YUV4MPEG2 W96 H64 F25:1 Ip A1:1 C420p10 XYSCSS=420P10"
    assert body == b"".join(b"FRAME\n" + vs._sr(f).astype("<u2").tobytes() for f in frames)
    back = y4m.Y4MReader(io.BytesIO(data), depths=(8, 10))
    assert (back.header.width, back.header.height, back.header.bits) == (96, 64, 10) and len(list(back)) == 4
    n, kw, data, vs = _run_upscale(_stream10(HEAD10, frames))                   # --bits 8: ten bits in, eight out
    assert kw["in_depth"] == 10 and kw["out_format"] == "i420" and data.startswith(b"YUV4MPEG2 W96 H64 F25:1 Ip A1:1 C420mpeg2\n")
    f8 = [np.random.default_rng(k).integers(0, 256, (24, 24)).astype(np.uint8) for k in range(2)]
    head8 = b"YUV4MPEG2 W24 H16 F25:1 Ip A1:1 C420mpeg2\n"
    n, kw, data, vs = _run_upscale(head8 + b"".join(b"FRAME\n" + f.tobytes() for f in f8), out_format="i010")
    assert n == 2 and "in_depth" not in kw and all(f.dtype == np.uint8 for f in vs.pushed)
    with pytest.raises(ValueError, match="header"):
        _run_upscale(_stream10(HEAD10, frames), in_depth=10)
    assert "10-bit source" in up.parser().format_help() and "--bits 10" in up.__doc__
