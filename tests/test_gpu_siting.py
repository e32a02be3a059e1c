"""Chroma siting on a real MI355X (include/pfnl_hip.h SITING; pfnl_amd/csrc/yuv.hip): both conversion kernels, at both depths, in all three
sitings, and the session's two edges, against the host rule pfnl_amd/yuv.py / pfnl_amd/depth10.py - byte for byte, no tolerance anywhere -
and the Y4M loop of pfnl_amd/upscale.py against the session driven directly."""
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfnl_amd import depth10, ops, surface, synth, y4m, yuv  # noqa: E402
from pfnl_amd import upscale as up  # noqa: E402
from pfnl_amd.engine import PFNLEngine  # noqa: E402
from pfnl_amd.spec import PFNLGeometry  # noqa: E402

PAIRS = [("bt601", False), ("bt709", True)]
# (2, 2), (2, 6), (6, 2): nothing but edges; (18, 34), (34, 66): single bytes, W / 2 odd; (10, 36): 4-byte words; (16, 64): 16-byte words
SHAPES = [(2, 2), (2, 6), (6, 2), (18, 34), (10, 36), (16, 64), (34, 66)]
SHAPES10 = [(2, 2), (6, 10), (16, 64)]                                  # edges; single samples; 16-byte words
H, W, BATCH, F = 16, 24, 2, 5                                           # the sessions: one block, sH x sW = 64 x 96


def _with_all_values(rng, shape, levels=256):
    a = rng.integers(0, levels, size=shape).astype(np.uint16 if levels > 256 else np.uint8)
    flat = a.reshape(-1)
    if flat.size >= levels:
        flat[rng.permutation(flat.size)[:levels]] = np.arange(levels)
        assert len(np.unique(flat)) == levels
    return a


def _extreme_blocks(rng, shape, top=255, block=2):
    """0 or ``top`` in blocks of ``block`` samples: every clip of either direction fires next to its opposite"""
    small = rng.integers(0, 2, size=tuple((s + block - 1) // block for s in shape[:2]) + tuple(shape[2:])) * top
    return np.repeat(np.repeat(small, block, axis=0), block, axis=1)[:shape[0], :shape[1]].astype(np.uint16 if top > 255 else np.uint8)


def _yuv_frames(n, h, w, fmt, seed):
    rng = np.random.default_rng(seed)
    frames = [_with_all_values(rng, (h * 3 // 2, w)) for _ in range(n)]
    if n > 1:
        frames[-1] = yuv.pack(_extreme_blocks(rng, (h, w)), _extreme_blocks(rng, (h // 2, w // 2)), _extreme_blocks(rng, (h // 2, w // 2)), fmt)
    return np.stack(frames)


def _rgb_frames(n, h, w, seed, levels=256):
    rng = np.random.default_rng(seed)
    frames = [_with_all_values(rng, (h, w, 3), levels) for _ in range(n)]
    if n > 1:
        frames[-1] = _extreme_blocks(rng, (h, w, 3), levels - 1)
    return np.stack(frames)


# ---- 1. the ops ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("siting", yuv.SITINGS)
@pytest.mark.parametrize("h,w", SHAPES)
def test_decode_equals_the_host_rule(h, w, siting):
    for fmt in yuv.FORMATS:
        for n in (1, 3):
            frames = _yuv_frames(n, h, w, fmt, seed=h * 1000 + w + n)
            dev = torch.from_numpy(frames).cuda()
            for matrix, full in PAIRS:
                got = ops.yuv420_to_rgb(dev, fmt, h, w, matrix, full, siting=siting).cpu().numpy()
                want = np.stack([yuv.to_rgb(f, fmt, h, w, matrix, full, siting=siting) for f in frames])
                assert got.dtype == np.uint8 and got.shape == want.shape == (n, h, w, 3)
                assert np.array_equal(got, want), (h, w, fmt, siting, n, matrix, full, int((got != want).sum()))
                if n > 1 and h * w >= 256:
                    assert want[-1].min() == 0 and want[-1].max() == 255                     # the extreme planes clip at both ends


@pytest.mark.parametrize("siting", yuv.SITINGS)
@pytest.mark.parametrize("h,w", SHAPES)
def test_encode_equals_the_host_rule(h, w, siting):
    for fmt in yuv.FORMATS:
        for n in (1, 3):
            frames = _rgb_frames(n, h, w, seed=h * 1000 + w + 10 + n)
            dev = torch.from_numpy(frames).cuda()
            for matrix, full in PAIRS:
                got = ops.rgb_to_yuv420(dev, fmt, matrix, full, siting=siting).cpu().numpy()
                want = np.stack([yuv.from_rgb(f, fmt, matrix, full, siting=siting) for f in frames])
                assert got.dtype == np.uint8 and got.shape == want.shape == (n, h * 3 // 2, w)
                assert np.array_equal(got, want), (h, w, fmt, siting, n, matrix, full, int((got != want).sum()))


@pytest.mark.parametrize("siting", yuv.SITINGS)
@pytest.mark.parametrize("h,w", SHAPES10)
def test_10_bit_encode_equals_the_host_rule(h, w, siting):
    for fmt in depth10.FORMATS:
        for n in (1, 3):
            frames = _rgb_frames(n, h, w, seed=h * 1000 + w + 20 + n, levels=1024)
            dev = torch.from_numpy(frames).cuda()
            for matrix, full in PAIRS:
                got = ops.rgb_to_yuv420_u10(dev, fmt, matrix, full, siting=siting).cpu().numpy()
                want = np.stack([depth10.from_rgb10(f, fmt, matrix, full, siting=siting) for f in frames])
                assert got.dtype == np.uint16 and got.shape == want.shape == (n, h * 3 // 2, w)
                assert np.array_equal(got, want), (h, w, fmt, siting, n, matrix, full, int((got != want).sum()))


@pytest.mark.parametrize("siting", yuv.SITINGS)
@pytest.mark.parametrize("h,w", [(16, 64), (10, 36)])          # shapes whose aligned form uses words: at an odd address it must not
def test_unaligned_pointers_take_the_byte_form_and_stay_inside_the_destination(h, w, siting):
    n, slack = 2, 64
    pattern = lambda size: (np.arange(size) * 7 + 3).astype(np.uint8)           # noqa: E731
    yb, rb = n * h * w * 3 // 2, n * h * w * 3
    for fmt in yuv.FORMATS:
        frames = _yuv_frames(n, h, w, fmt, seed=5)
        rgbs = _rgb_frames(n, h, w, seed=6)
        for off in (1, 4):                                                      # single bytes; 4-byte words at most
            src = torch.zeros(off + yb, dtype=torch.uint8, device="cuda")
            src[off:] = torch.from_numpy(frames.reshape(-1)).cuda()
            pat = pattern(slack + off + rb + slack)
            dst = torch.from_numpy(pat).cuda()
            ops.yuv420_to_rgb(src[off:], fmt, h, w, "bt601", False, out=dst[slack + off:slack + off + rb], siting=siting)
            got = dst.cpu().numpy()
            want = np.stack([yuv.to_rgb(f, fmt, h, w, "bt601", False, siting=siting) for f in frames])
            assert np.array_equal(got[slack + off:slack + off + rb].reshape(want.shape), want), (fmt, off)
            assert np.array_equal(got[:slack + off], pat[:slack + off]) and np.array_equal(got[slack + off + rb:], pat[slack + off + rb:])
            src = torch.zeros(off + rb, dtype=torch.uint8, device="cuda")
            src[off:] = torch.from_numpy(rgbs.reshape(-1)).cuda()
            pat = pattern(slack + off + yb + slack)
            dst = torch.from_numpy(pat).cuda()
            ops.rgb_to_yuv420(src[off:].view(n, h, w, 3), fmt, "bt601", False, out=dst[slack + off:slack + off + yb], siting=siting)
            got = dst.cpu().numpy()
            want = np.stack([yuv.from_rgb(f, fmt, "bt601", False, siting=siting) for f in rgbs])
            assert np.array_equal(got[slack + off:slack + off + yb].reshape(want.shape), want), (fmt, off)
            assert np.array_equal(got[:slack + off], pat[:slack + off]) and np.array_equal(got[slack + off + yb:], pat[slack + off + yb:])


@pytest.mark.parametrize("siting", ["center", "topleft"])
@pytest.mark.parametrize("fmt", yuv.FORMATS)
def test_surface_decode_with_a_pitch_above_the_width(fmt, siting):
    h, w = 18, 34
    for frame in _yuv_frames(2, h, w, fmt, seed=77):
        planes = surface.split(frame, fmt, h, w)
        for pitches in ([p.shape[1] + 1 for p in planes], [(p.shape[1] + 63) // 64 * 64 + 64 for p in planes]):
            outs = []
            for fill in (0x00, 0xFF):                                           # what lies between a row's end and the pitch never counts
                bufs = [torch.from_numpy(b).cuda() for b in surface.embed(planes, pitches, fill)]
                views = surface.views(bufs, fmt, h, w)
                assert surface.describe(views, fmt, h, w)[1] == pitches
                outs.append(ops.yuv420_to_rgb_surface(views, fmt, h, w, "bt709", False, siting=siting).cpu().numpy())
            want = yuv.to_rgb(frame, fmt, h, w, "bt709", False, siting=siting)
            assert np.array_equal(outs[0], want) and np.array_equal(outs[1], want), (fmt, siting, pitches)


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


def _i420_sequence(seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (H * 3 // 2, W), dtype=np.uint8) for _ in range(F)]


@pytest.fixture(scope="module")
def rgb_reference(engines):
    """(the I420 frames, the default RGB session's SR frames for to_rgb(frame, siting="center")): computed once, read by several tests"""
    frames = _i420_sequence(3)
    with engines[1].open_stream(H, W, BATCH) as vs:
        sr = _stream_all(vs, [yuv.to_rgb(f, "i420", H, W, "bt601", False, siting="center") for f in frames])
    sr.setflags(write=False)
    return frames, sr


def test_center_sited_input_equals_the_rgb_session_fed_the_host_decode(engines, rgb_reference):
    frames, want = rgb_reference
    with engines[0].open_stream(H, W, BATCH, pixel_format="i420", out_format="rgb24", matrix="bt601", chroma_siting="center") as vs:
        assert (vs.chroma_siting, vs.out_chroma_siting) == ("center", "center")
        for device in (False, True):
            got = _stream_all(vs, frames, device)
            assert got.shape == (F, 4 * H, 4 * W, 3) and np.array_equal(got, want), (device, int((got != want).sum()))
            vs.reset()                                                          # the siting survives
    left = np.stack([yuv.to_rgb(f, "i420", H, W, "bt601", False) for f in frames])
    assert not np.array_equal(left, np.stack([yuv.to_rgb(f, "i420", H, W, "bt601", False, siting="center") for f in frames]))


def test_topleft_sited_output_equals_the_host_encode_of_the_rgb_sessions_frames(engines):
    rgb = list(np.random.default_rng(4).integers(0, 256, (F, H, W, 3), dtype=np.uint8))
    with engines[1].open_stream(H, W, BATCH) as vs:
        sr = _stream_all(vs, rgb)
    want = np.stack([yuv.from_rgb(f, "i420", "bt709", False, siting="topleft") for f in sr])
    with engines[0].open_stream(H, W, BATCH, out_format="i420", out_chroma_siting="topleft") as vs:
        assert (vs.chroma_siting, vs.out_chroma_siting) == ("left", "topleft")
        for device in (False, True):
            got = _stream_all(vs, rgb, device)
            assert got.shape == (F, 4 * H * 3 // 2, 4 * W) and np.array_equal(got, want), (device, int((got != want).sum()))
            vs.reset()
    assert not np.array_equal(want, np.stack([yuv.from_rgb(f, "i420", "bt709", False) for f in sr]))


def test_left_by_keyword_is_the_session_without_the_keyword(engines):
    frames = _i420_sequence(5)
    with engines[0].open_stream(H, W, BATCH, pixel_format="i420") as vs:
        plain = _stream_all(vs, frames)
    with engines[0].open_stream(H, W, BATCH, pixel_format="i420", chroma_siting="left") as vs:
        assert (vs.chroma_siting, vs.out_chroma_siting) == ("left", "left")
        assert np.array_equal(_stream_all(vs, frames), plain)
    with engines[0].open_stream(H, W, BATCH, pixel_format="i420", chroma_siting="left", out_chroma_siting="left") as vs:
        assert np.array_equal(_stream_all(vs, frames, device=True), plain)
    for bad in ({"chroma_siting": "centre"}, {"out_chroma_siting": 1}):         # refused before anything touches the engine
        with pytest.raises(ValueError):
            engines[0].open_stream(H, W, BATCH, pixel_format="i420", **bad)
    with engines[0].open_stream(H, W, BATCH, pixel_format="i420", chroma_siting="center") as vs:
        lib = vs._lib
        vs.push(frames[0])
        assert lib.pfnl_stream_chroma_siting(vs._s, 0, 0) == -2 and b"before the first frame" in lib.pfnl_last_error()   # PFNL_ERR_STATE
        assert lib.pfnl_stream_chroma_siting(vs._s, 3, 0) == -1


def test_planes_follow_the_sessions_sitings(engines, rgb_reference):
    """push_planes of pitched NV12 device surfaces and pop_planes into one, centre-sited on both sides: the samples are from_rgb(centre) of
    the RGB session's frames for to_rgb(centre) of the input, and nothing else of the destination is written."""
    frames, sr = rgb_reference
    want = [yuv.from_rgb(f, "nv12", "bt601", False, siting="center") for f in sr]
    oH, oW = 4 * H, 4 * W
    out_pitches = [oW + 64, oW + 32]
    got = []
    with engines[0].open_stream(H, W, BATCH, pixel_format="nv12", matrix="bt601", chroma_siting="center") as vs:
        def drain():
            while vs.ready():
                bufs = [torch.full((rows, pitch), 0xA5, dtype=torch.uint8, device="cuda") for rows, pitch in zip((oH, oH // 2), out_pitches)]
                views = surface.views(bufs, "nv12", oH, oW)
                index = vs.pop_planes(*views)
                assert index == len(got)
                host = [b.cpu().numpy() for b in bufs]
                assert all((b[:, oW:] == 0xA5).all() for b in host)
                got.append(yuv.pack(host[0][:, :oW], host[1][:, 0:oW:2], host[1][:, 1:oW:2], "nv12"))

        for f in frames:
            planes = surface.split(yuv.pack(*yuv.planes(f, "i420", H, W), "nv12"), "nv12", H, W)
            bufs = [torch.from_numpy(b).cuda() for b in surface.embed(planes, [W + 40, W + 8], 0x3C)]
            assert vs.push_planes(*surface.views(bufs, "nv12", H, W)) == []      # (everything deliverable was popped before)
            drain()
        vs._lib.pfnl_stream_end(vs._handle())
        drain()
    assert len(got) == F and all(np.array_equal(g, w_) for g, w_ in zip(got, want))


# ---- 3. Y4M end to end ----------------------------------------------------------------------------------------------------------------------
def _y4m_bytes(header, frames):
    return header + b"".join(b"FRAME\n" + f.tobytes() for f in frames)


def test_upscale_equals_the_session_driven_directly(engines):
    frames = _i420_sequence(8)
    data = _y4m_bytes(b"YUV4MPEG2 W24 H16 F25:1 Ip A1:1 C420jpeg\n", frames)
    out, log = io.BytesIO(), io.StringIO()
    assert up.upscale(y4m.Y4MReader(io.BytesIO(data)), y4m.Y4MWriter(out), engines[0].open_stream, batch=BATCH, log=log) == F
    with engines[1].open_stream(H, W, BATCH, pixel_format="i420", out_format="i420", matrix="bt601", full_range=False,
                                chroma_siting="center") as vs:
        want = _stream_all(vs, frames)
    head, body = out.getvalue().split(b"\n", 1)
    assert head == b"YUV4MPEG2 W96 H64 F25:1 Ip A1:1 C420jpeg"
    assert body == b"".join(b"FRAME\n" + f.tobytes() for f in want)
    assert log.getvalue().startswith(f"pfnl_amd.upscale: {F} frames in ")


def test_command_line_at_10_bits_on_a_canvas(engines, tmp_path):
    frames = _i420_sequence(9)
    src, dst = tmp_path / "in.y4m", tmp_path / "out.y4m"
    src.write_bytes(_y4m_bytes(b"YUV4MPEG2 W24 H16 F25:1 Ip A16:15 C420jpeg\n", frames))
    assert up.main([str(src), str(dst), "--synthetic-weights", "0", "--num-block", "1", "--batch", str(BATCH), "--bits", "10", "--out-size", "72x100",
                    "--fit", "contain"]) == 0
    with engines[1].open_stream(H, W, BATCH, pixel_format="i420", out_format="i010", matrix="bt601", full_range=False, out_size=(72, 100),
                                fit="contain", sar=(16, 15), chroma_siting="center") as vs:
        want = _stream_all(vs, frames)
    assert want.dtype == np.uint16 and want.shape == (F, 72 * 3 // 2, 100)
    head, body = dst.read_bytes().split(b"\n", 1)
    assert head == b"YUV4MPEG2 W100 H72 F25:1 Ip A1:1 C420p10 XYSCSS=420P10"
    assert body == b"".join(b"FRAME\n" + f.astype("<u2").tobytes() for f in want)
