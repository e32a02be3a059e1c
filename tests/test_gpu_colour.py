"""Colour per side on a real MI355X (include/pfnl_hip.h COLOUR; pfnl_amd/csrc/colour.hip): the colour stage 0 on its own and inside the
session, against the host rule pfnl_amd/colour.py - sample for sample, no tolerance anywhere - and the Y4M loop of pfnl_amd/upscale.py
against the session driven directly."""
import ctypes as C
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfnl_amd import _capi, colour, depth10, ops, packed, resize, synth, y4m, yuv  # noqa: E402
from pfnl_amd import upscale as up  # noqa: E402
from pfnl_amd.engine import PFNLEngine  # noqa: E402
from pfnl_amd.spec import PFNLGeometry  # noqa: E402

PAIRS = [(s, d) for s in colour.PRIMARIES for d in colour.PRIMARIES if s != d]
SWEEP = 1024 * 256 * 4                                                   # the pixels of one sweep of the launch's grid: it strides beyond
COUNTS = [4, 12, 4 * 257, SWEEP + 4 * 259]                               # one lane; three; a partial wave and a second workgroup; a second sweep
H, W, BATCH, F = 16, 24, 2, 5                                            # the sessions: one block, sH x sW = 64 x 96


def _levels(x, top):
    """what both quantise kernels compute: the float32 product, clipped, rounded half to even; NaN -> 0"""
    v = np.clip(x.astype(np.float32) * np.float32(top), np.float32(0), np.float32(top))
    return np.round(np.where(np.isnan(v), np.float32(0), v)).astype(np.uint8 if top == 255 else np.uint16)


@pytest.fixture(scope="module")
def pool():
    """[COUNTS[-1], 3] float32 on both sides, shared and unchanged: the saturated primaries and their mixes, NaN, values outside 0 .. 1, the
    grey ramp of both depths, then random values in [-0.1, 1.1]"""
    rng = np.random.default_rng(7)
    x = rng.uniform(-0.1, 1.1, (COUNTS[-1], 3)).astype(np.float32)
    x[:8] = [[(k >> 2) & 1, (k >> 1) & 1, k & 1] for k in range(8)]
    x[8] = np.nan
    x[9] = [np.nan, 0.5, 1.0]
    x[10] = [-3.0, 7.0, np.inf]
    x[11] = [0.25, -np.inf, 0.75]
    x[12:12 + 256] = (np.arange(256, dtype=np.float32) / np.float32(255))[:, None]
    x[2048:2048 + 1024] = (np.arange(1024, dtype=np.float32) / np.float32(1023))[:, None]
    x.setflags(write=False)
    return x, torch.from_numpy(x.copy()).cuda()


# ---- 1. the hooks -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("n", COUNTS)
def test_the_hook_equals_the_host_rule(pool, n, bits):
    host, dev = pool
    q = _levels(host[:n], (1 << bits) - 1)
    plain = (ops.quantise_u8 if bits == 8 else ops.quantise_u10)(dev[:n]).cpu().numpy()
    assert np.array_equal(plain, q)                                      # the levels are the plain quantise's
    if n >= 12:
        assert q[8].tolist() == [0, 0, 0] and q[10].tolist() == [0, (1 << bits) - 1, (1 << bits) - 1]
    for s in colour.PRIMARIES:                                           # no conversion: pfnl_op_quantise_* itself
        assert np.array_equal(ops.quantise_colour(dev[:n], s, s, bits).cpu().numpy(), plain), s
    for s, d in PAIRS:
        got = ops.quantise_colour(dev[:n], s, d, bits).cpu().numpy()
        want = colour.convert(q, s, d, bits)
        assert got.dtype == want.dtype and got.shape == (n, 3)
        assert np.array_equal(got, want), (s, d, n, bits, int((got != want).sum()))
        assert not np.array_equal(got[:8], plain[:8])                    # the saturated colours move
        if n > 12 + 256:
            assert np.array_equal(got[12:12 + 256], plain[12:12 + 256])  # the greys do not


def test_the_hook_writes_its_samples_and_nothing_else(pool):
    _, dev = pool
    n = 4 * 257
    for bits in (8, 10):
        whole = torch.from_numpy(np.full((n + 16, 3), 0xA5 if bits == 8 else 0xA5A5, np.uint8 if bits == 8 else np.uint16)).cuda()
        ops.quantise_colour(dev[:n], "bt601-525", "bt709", bits, out=whole[8:8 + n])
        got = whole.cpu().numpy()
        assert (got[:8] == got[0, 0]).all() and (got[8 + n:] == got[0, 0]).all()
        assert np.array_equal(got[8:8 + n], ops.quantise_colour(dev[:n], "bt601-525", "bt709", bits).cpu().numpy())


def test_the_hook_refuses():
    lib = _capi.load_library()
    x = torch.zeros((16, 3), dtype=torch.float32, device="cuda")
    for bits in (8, 10):
        with pytest.raises(_capi.PFNLHipError, match="multiple of 4"):
            ops.quantise_colour(x[:6], "bt709", "bt601-525", bits)
        with pytest.raises(_capi.PFNLHipError, match="aligned"):
            ops.quantise_colour(x.view(-1)[3:15].view(4, 3), "bt709", "bt601-525", bits)                  # sr at 12 bytes
        out = torch.zeros((9, 3), dtype=torch.uint8 if bits == 8 else torch.uint16, device="cuda")
        with pytest.raises(_capi.PFNLHipError, match="aligned"):
            ops.quantise_colour(x[:8], "bt709", "bt601-525", bits, out=out.view(-1)[3:27].view(8, 3))     # out at 3 or 6 bytes
        with pytest.raises(ValueError):
            ops.quantise_colour(x, "bt2020", "bt709", bits)
        with pytest.raises(ValueError):
            ops.quantise_colour(x.view(12, 4), "bt709", "bt601-525", bits)                                # pixels are [..., 3]
        hook = lib.pfnl_op_quantise_colour_u8 if bits == 8 else lib.pfnl_op_quantise_colour_u10
        assert hook(C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), 4, 0, 3, None) == -1 and b"primaries" in lib.pfnl_last_error()
    with pytest.raises(ValueError):
        ops.quantise_colour(x, "bt709", "bt601-525", 12)


# ---- 2. the session -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engines():
    geom = PFNLGeometry(num_block=1)
    w = synth.synthetic_weights(geom, seed=0)
    made = []
    for _ in range(2):
        e = PFNLEngine(geom, device=0)
        e.load_weights(w)
        made.append(e)
    yield made
    for e in made:
        e.close()


def _stream_all(vs, frames, device=False):
    got = []
    for f in frames:
        got += vs.push(torch.from_numpy(f).cuda() if device else f)
        got += vs.pop_ready()
    got += vs.end()
    got = [(i, f.cpu().numpy() if torch.is_tensor(f) else f) for i, f in got]
    assert [i for i, _ in got] == list(range(len(frames)))
    return np.stack([f for _, f in got])


def _i420_sequence(seed, h=H, w=W, n=F):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h * 3 // 2, w), dtype=np.uint8) for _ in range(n)]


SD = dict(pixel_format="i420", matrix="bt601", primaries="bt601-525")    # the input side of the sessions: a DVD's
HD = dict(out_matrix="bt709", out_primaries="bt709")                     # the output side: what an HD stream is read as


@pytest.fixture(scope="module")
def reference(engines):
    """(the I420 frames, P: what an out_format="rgb24" session without the setting delivers for them): computed once, read by several tests"""
    frames = _i420_sequence(3)
    with engines[1].open_stream(H, W, BATCH, pixel_format="i420", out_format="rgb24", matrix="bt601") as vs:
        P = _stream_all(vs, frames)
    assert P.shape == (F, 4 * H, 4 * W, 3) and P.min() != P.max()
    P.setflags(write=False)
    return frames, P


def test_sd_in_hd_out_equals_the_host_rule_on_the_plain_sessions_frames(engines, reference):
    frames, P = reference
    moved = colour.convert(P, "bt601-525", "bt709")
    assert not np.array_equal(moved, P)
    want = np.stack([yuv.from_rgb(f, "i420", "bt709", False) for f in moved])
    with engines[0].open_stream(H, W, BATCH, **SD, **HD) as vs:
        assert (vs.matrix, vs.out_matrix, vs.full_range, vs.out_full_range, vs.primaries, vs.out_primaries) == \
            ("bt601", "bt709", False, False, "bt601-525", "bt709")
        for device in (False, True):
            got = _stream_all(vs, frames, device)
            assert got.shape == want.shape and np.array_equal(got, want), (device, int((got != want).sum()))
            vs.reset()                                                   # the setting survives
    assert not np.array_equal(want, np.stack([yuv.from_rgb(f, "i420", "bt709", False) for f in P]))


def test_matrix_and_range_alone_change_the_output_conversion_only(engines, reference):
    frames, P = reference
    want = np.stack([yuv.from_rgb(f, "i420", "bt709", True) for f in P])
    with engines[0].open_stream(H, W, BATCH, pixel_format="i420", matrix="bt601", out_matrix="bt709", out_full_range=True) as vs:
        assert (vs.primaries, vs.out_primaries, vs.out_full_range) == ("bt709", "bt709", True)
        got = _stream_all(vs, frames)
    assert np.array_equal(got, want), int((got != want).sum())
    with engines[0].open_stream(H, W, BATCH, **SD, out_primaries="bt601-525", out_format="rgb24") as vs:   # equal primaries: the frames as they are
        assert np.array_equal(_stream_all(vs, frames), P)


def test_everything_behind_stage_0_sees_the_output_colours(engines, reference):
    frames, P = reference
    moved = colour.convert(P, "bt601-525", "bt709")
    oH, oW = 40, 72
    want = np.stack([yuv.from_rgb(resize.resize(f, oH, oW), "i420", "bt709", False) for f in moved])
    with engines[0].open_stream(H, W, BATCH, **SD, **HD, out_size=(oH, oW)) as vs:                         # the converted frames, resized
        got = _stream_all(vs, frames)
    assert got.shape == (F, oH * 3 // 2, oW) and np.array_equal(got, want), int((got != want).sum())
    want = np.stack([packed.from_rgb(f, "bgra") for f in moved])
    with engines[0].open_stream(H, W, BATCH, **SD, out_primaries="bt709", out_format="rgb24", out_packing="bgra") as vs:   # ... packed
        got = _stream_all(vs, frames, device=True)
    assert np.array_equal(got.reshape(want.shape), want), int((got.reshape(want.shape) != want).sum())


def test_ten_bits_out(engines):
    rgb = list(np.random.default_rng(4).integers(0, 256, (F, H, W, 3), dtype=np.uint8))
    with engines[1].open_stream(H, W, BATCH, out_format="rgb10") as vs:
        P10 = _stream_all(vs, rgb)
    assert P10.dtype == np.uint16 and int(P10.max()) <= 1023
    moved = colour.convert(P10, "bt601-625", "bt709", 10)
    assert not np.array_equal(moved, P10)
    want = np.stack([depth10.from_rgb10(f, "p010", "bt709", False) for f in moved])
    with engines[0].open_stream(H, W, BATCH, out_format="p010", primaries="bt601-625", out_primaries="bt709") as vs:
        got = _stream_all(vs, rgb)
        assert got.dtype == np.uint16 and np.array_equal(got, want), int((got != want).sum())
        vs.reset()
        assert np.array_equal(_stream_all(vs, rgb, device=True), want)


def test_a_later_format_call_replaces_matrix_and_range_and_leaves_the_primaries(engines, reference):
    frames, P = reference
    with engines[1].open_stream(H, W, BATCH, pixel_format="i420", out_format="rgb24", matrix="bt601", full_range=True) as ref:
        P2 = _stream_all(ref, frames)                                    # the frames decoded at (bt601, full)
    assert not np.array_equal(P2, P)
    moved = colour.convert(P2, "bt601-525", "bt709")
    with engines[0].open_stream(H, W, BATCH, **SD, **HD) as vs:
        lib, i420 = vs._lib, _capi.PIXEL_FORMATS["i420"]
        _capi.check(lib.pfnl_stream_format(vs._s, i420, i420, 0, 1))     # both sides now convert at (bt601, full); the primaries are what they were
        want = np.stack([yuv.from_rgb(f, "i420", "bt601", True) for f in moved])
        got = _stream_all(vs, frames)
        assert np.array_equal(got, want), int((got != want).sum())
        vs.reset()                                                       # and the colour call replaces what the format call set, one side at a time
        side = _capi.pfnl_colour(1, 0, 0)                                # the output: BT.709, limited, BT.709 primaries
        _capi.check(lib.pfnl_stream_colour(vs._s, None, C.byref(side)))
        want = np.stack([yuv.from_rgb(f, "i420", "bt709", False) for f in moved])
        got = _stream_all(vs, frames)
        assert np.array_equal(got, want), int((got != want).sum())


def test_the_setter_refuses_and_changes_nothing(engines, reference):
    frames, P = reference
    want = np.stack([yuv.from_rgb(f, "i420", "bt709", False) for f in colour.convert(P, "bt601-525", "bt709")])
    with engines[0].open_stream(H, W, BATCH, **SD, **HD) as vs:
        lib = vs._lib
        good = _capi.pfnl_colour(0, 0, 2)
        for bad in ((2, 0, 0), (0, 2, 0), (0, 0, 3), (-1, 0, 0), (0, 0, -1)):
            side = _capi.pfnl_colour(*bad)
            assert lib.pfnl_stream_colour(vs._s, C.byref(good), C.byref(side)) == -1 and b"colour" in lib.pfnl_last_error()   # PFNL_ERR_INVALID
            assert lib.pfnl_stream_colour(vs._s, C.byref(side), None) == -1
        assert lib.pfnl_stream_colour(vs._s, None, None) == 0
        vs.push(frames[0])
        assert lib.pfnl_stream_colour(vs._s, C.byref(good), None) == -2 and b"before the first frame" in lib.pfnl_last_error()   # PFNL_ERR_STATE
        vs.reset()
        assert np.array_equal(_stream_all(vs, frames), want)             # neither the refused values nor `good` reached the setting
    for bad in ({"out_primaries": "bt2020"}, {"primaries": 1}, {"out_matrix": "bt2020"}):     # refused before anything touches the engine
        with pytest.raises(ValueError):
            engines[0].open_stream(H, W, BATCH, pixel_format="i420", **bad)


def test_the_keywords_at_their_defaults_are_the_session_without_them(engines):
    frames = _i420_sequence(5)
    with engines[0].open_stream(H, W, BATCH, pixel_format="i420", matrix="bt601", full_range=True) as vs:
        plain = _stream_all(vs, frames)
    with engines[0].open_stream(H, W, BATCH, pixel_format="i420", matrix="bt601", full_range=True, out_matrix=None, out_full_range=None,
                                primaries="bt709", out_primaries=None) as vs:
        assert (vs.out_matrix, vs.out_full_range, vs.primaries, vs.out_primaries) == ("bt601", True, "bt709", "bt709")
        assert np.array_equal(_stream_all(vs, frames), plain)
    with engines[0].open_stream(H, W, BATCH, pixel_format="i420", matrix="bt601", full_range=True, out_matrix="bt601", out_full_range=True,
                                out_primaries="bt709") as vs:            # the same setting, through the new entry
        assert np.array_equal(_stream_all(vs, frames, device=True), plain)


# ---- 3. Y4M end to end ----------------------------------------------------------------------------------------------------------------------
def test_upscale_of_a_480_line_stream_equals_the_session_driven_directly(engines):
    h, w, n = 480, 24, 3
    frames = _i420_sequence(8, h, w, n)
    data = b"YUV4MPEG2 W24 H480 F30000:1001 Ip A10:11 C420mpeg2\n" + b"".join(b"FRAME\n" + f.tobytes() for f in frames)
    out, log = io.BytesIO(), io.StringIO()
    assert up.upscale(y4m.Y4MReader(io.BytesIO(data)), y4m.Y4MWriter(out), engines[0].open_stream, batch=BATCH, log=log, out_matrix="auto",
                      primaries="auto", out_primaries="auto") == n
    with engines[1].open_stream(h, w, BATCH, pixel_format="i420", out_format="i420", matrix="bt601", full_range=False, primaries="bt601-525",
                                out_matrix="bt709", out_primaries="bt709") as vs:
        want = _stream_all(vs, frames)
    with engines[1].open_stream(h, w, BATCH, pixel_format="i420", out_format="i420", matrix="bt601") as vs:
        assert not np.array_equal(_stream_all(vs, frames), want)         # what the stream was written as before: BT.601 under an HD raster
    head, body = out.getvalue().split(b"\n", 1)
    assert head == b"YUV4MPEG2 W96 H1920 F30000:1001 Ip A10:11 C420mpeg2"
    assert body == b"".join(b"FRAME\n" + f.tobytes() for f in want)
