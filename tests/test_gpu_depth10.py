"""10-bit output on a real MI355X (include/pfnl_hip.h pfnl_stream_format with PFNL_PIX_RGB10 / P010 / I010; pfnl_amd/csrc/depth10.hip): the
three kernels and the session's output edge against the host rule pfnl_amd/depth10.py, sample for sample - no tolerance anywhere but in the
comparison of the 10-bit picture with the 8-bit one, where the bound is the two roundings'."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfnl_amd import depth10, ops, synth, yuv  # noqa: E402
from pfnl_amd import model as M  # noqa: E402
from pfnl_amd.engine import PFNLEngine  # noqa: E402
from pfnl_amd.spec import PFNLGeometry  # noqa: E402

PAIRS = [("bt601", False), ("bt601", True), ("bt709", False), ("bt709", True)]
# (2, 2): nothing but edges; (4, 6), (18, 50): single samples, W / 2 odd, several strips; (16, 24), (32, 64): 16-byte words (W % 8 == 0)
SHAPES = [(2, 2), (4, 6), (16, 24), (18, 50), (32, 64)]
# the nine geometries of tests/test_gpu_resize.py; 16-byte stores where oW % 8 == 0: (16, 24) twice, (64, 96) -> (16, 24) and -> (128, 192)
GEOMETRIES = [((8, 8), (2, 2)), ((16, 24), (16, 24)), ((16, 24), (9, 13)), ((64, 96), (36, 54)), ((64, 96), (16, 24)), ((64, 96), (128, 192)),
              ((48, 80), (90, 100)), ((40, 200), (30, 75)), ((20, 600), (10, 333))]


def _dev16(a):
    """a uint16 numpy array on the device as torch.uint16 (through int16: the copy kernels all know that type)"""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda().view(torch.uint16)


def _host16(t):
    assert t.dtype == torch.uint16
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _samples_with_all_values(rng, shape):
    a = rng.integers(0, 1024, size=shape, dtype=np.uint16)
    flat = a.reshape(-1)
    if flat.size >= 1024:
        flat[rng.permutation(flat.size)[:1024]] = np.arange(1024, dtype=np.uint16)
        assert len(np.unique(flat)) == 1024
    return a


def _extreme_blocks(rng, shape, block=2):
    """0 or 1023 in blocks of `block` samples: every clip of either direction fires next to its opposite"""
    small = rng.integers(0, 2, size=tuple((s + block - 1) // block for s in shape[:2]) + tuple(shape[2:]), dtype=np.uint16) * 1023
    return np.repeat(np.repeat(small, block, axis=0), block, axis=1)[:shape[0], :shape[1]]


def _rgb10_frames(n, H, W, seed):
    """n frames of random samples with every value present (where they fit); the last one 0 / 1023 blocks of 2 x 2"""
    rng = np.random.default_rng(seed)
    frames = [_samples_with_all_values(rng, (H, W, 3)) for _ in range(n)]
    frames[-1] = _extreme_blocks(rng, (H, W, 3))
    return np.stack(frames)


def _guarded(op, src_np, out_samples, off, slack=64):
    """runs op(src, out) with both tensors `off` samples behind an aligned address and a pattern around the destination: (result, intact)"""
    pattern = ((np.arange(slack + off + out_samples + slack) * 7 + 3) % 65536).astype(np.uint16)
    src = torch.zeros(off + src_np.size, dtype=torch.int16, device="cuda")
    src[off:] = torch.from_numpy(src_np.reshape(-1).view(np.int16)).cuda()
    dst = _dev16(pattern)
    lo = slack + off
    assert (src.data_ptr() + 2 * off) % 16 == (2 * off) % 16 and (dst.data_ptr() + 2 * lo) % 16 == (2 * off) % 16
    op(src.view(torch.uint16)[off:], dst[lo:lo + out_samples])
    got = _host16(dst)
    intact = np.array_equal(got[:lo], pattern[:lo]) and np.array_equal(got[lo + out_samples:], pattern[lo + out_samples:])
    return got[lo:lo + out_samples], intact


# ---- 1. quantise ------------------------------------------------------------------------------------------------------------------------
def test_quantise_u10_equals_the_host_rule():
    rng = np.random.default_rng(1)
    x = rng.uniform(-0.1, 1.1, 1 << 16).astype(np.float32)
    x[:6] = [0.0, -0.0, 1.0, np.inf, -np.inf, np.float32(np.nextafter(np.float32(1.0), np.float32(2.0)))]
    t = ((np.arange(1023) + 0.5) / 1023).astype(np.float32)                    # the ties of every pair of neighbouring codes, and the floats around them
    below, above = np.nextafter(t, np.float32(-1)), np.nextafter(t, np.float32(2))
    x = np.concatenate([x, below, t, above, np.nextafter(above, np.float32(2))])
    assert x.dtype == np.float32 and x.size == (1 << 16) + 4 * 1023
    want = depth10.quantise10(x)
    assert len(np.unique(want)) == 1024 and (want[(1 << 16):(1 << 16) + 1023] <= want[(1 << 16) + 3 * 1023:]).all()
    got = ops.quantise_u10(torch.from_numpy(x).cuda())
    assert got.dtype == torch.uint16 and tuple(got.shape) == x.shape
    got = _host16(got)
    assert np.array_equal(got, want), int((got != want).sum())
    with pytest.raises(Exception):
        ops.quantise_u10(torch.zeros(6, device="cuda"))                         # n % 4


# ---- 2. RGB -> 4:2:0 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", depth10.FORMATS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_rgb_to_yuv420_u10_equals_the_host_rule(H, W, fmt):
    for n in (1, 3):
        frames = _rgb10_frames(n, H, W, seed=H * 1000 + W + n)
        dev = _dev16(frames)
        for matrix, full in PAIRS:
            got = ops.rgb_to_yuv420_u10(dev, fmt, matrix, full)
            assert got.dtype == torch.uint16
            got = _host16(got)
            want = np.stack([depth10.from_rgb10(f, fmt, matrix, full) for f in frames])
            assert got.shape == want.shape == (n, H * 3 // 2, W)
            assert np.array_equal(got, want), (H, W, fmt, n, matrix, full, int((got != want).sum()))
            if fmt == "p010":
                assert not (got & 63).any()
    single = ops.rgb_to_yuv420_u10(_dev16(frames[0]), fmt, "bt601", True)       # [H,W,3] is a batch of one
    assert tuple(single.shape) == (1, H * 3 // 2, W) and np.array_equal(_host16(single)[0], depth10.from_rgb10(frames[0], fmt, "bt601", True))


@pytest.mark.parametrize("fmt", depth10.FORMATS)
@pytest.mark.parametrize("H,W", [(16, 24), (18, 50)])          # the first uses words where it may: at an address that is not 16-byte aligned it must not
def test_yuv_unaligned_pointers_take_the_narrow_form_and_stay_inside_the_destination(H, W, fmt):
    n = 2
    frames = _rgb10_frames(n, H, W, seed=6)
    want = np.stack([depth10.from_rgb10(f, fmt, "bt601", False) for f in frames])
    for off in (0, 1, 2):                                                       # in samples: 0 keeps the words, and they end where the frames end
        got, intact = _guarded(lambda s, d: ops.rgb_to_yuv420_u10(s.view(n, H, W, 3), fmt, "bt601", False, out=d), frames, want.size, off)
        assert np.array_equal(got.reshape(want.shape), want), (H, W, fmt, off)
        assert intact, (H, W, fmt, off)


def test_yuv_wrong_arguments_raise():
    x = torch.zeros((2, 16, 24, 3), dtype=torch.uint16, device="cuda")
    for bad in ("nv12", "rgb10", "P010"):
        with pytest.raises(ValueError):
            ops.rgb_to_yuv420_u10(x, bad)
    with pytest.raises(ValueError):
        ops.rgb_to_yuv420_u10(x, "p010", "bt2020")
    with pytest.raises(ValueError):
        ops.rgb_to_yuv420_u10(torch.zeros((2, 15, 24, 3), dtype=torch.uint16, device="cuda"), "p010")
    with pytest.raises(ValueError):
        ops.rgb_to_yuv420_u10(x, "p010", out=torch.zeros(5, dtype=torch.uint16, device="cuda"))
    with pytest.raises(TypeError):
        ops.rgb_to_yuv420_u10(x.view(torch.int16), "p010")
    with pytest.raises(TypeError):
        ops.rgb_to_yuv420_u10(x.cpu(), "p010")


# ---- 3. resize --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,out", GEOMETRIES)
def test_resize_u10_equals_the_host_rule(size, out):
    (H, W), (oH, oW) = size, out
    for n in (1, 3):
        frames = _rgb10_frames(n, H, W, seed=H * 1000 + W + n)
        want = np.stack([depth10.resize10(f, oH, oW) for f in frames])
        got = ops.resize_u10(_dev16(frames), (oH, oW))
        assert got.dtype == torch.uint16
        got = _host16(got)
        assert got.shape == want.shape == (n, oH, oW, 3)
        assert np.array_equal(got, want), (size, out, n, int((got != want).sum()))
        if (H, W) != (oH, oW) and H * W >= 256:                                 # the block frame overshoots, and the clip removes it, at both ends
            raw = depth10.resize10_unclipped(frames[-1], oH, oW)
            assert raw.min() < 0 and raw.max() > 1023
            assert want[-1].min() == 0 and want[-1].max() == 1023
    single = ops.resize_u10(_dev16(frames[0]), (oH, oW))                        # [H,W,3] is a batch of one
    assert tuple(single.shape) == (1, oH, oW, 3) and np.array_equal(_host16(single)[0], want[0])


@pytest.mark.parametrize("size,out", [((64, 96), (128, 192)), ((16, 24), (9, 13)), ((8, 8), (2, 2))])   # 16-byte stores; an odd width; all clamped
def test_resize_unaligned_pointers_take_the_sample_form_and_stay_inside_the_destination(size, out):
    (H, W), (oH, oW) = size, out
    n = 2
    frames = _rgb10_frames(n, H, W, seed=7)
    want = np.stack([depth10.resize10(f, oH, oW) for f in frames])
    for off in (0, 1, 2):
        got, intact = _guarded(lambda s, d: ops.resize_u10(s.view(n, H, W, 3), (oH, oW), out=d), frames, want.size, off)
        assert np.array_equal(got.reshape(want.shape), want), (size, out, off)
        assert intact, (size, out, off)


def test_resize_wrong_arguments_raise():
    x = torch.zeros((2, 16, 24, 3), dtype=torch.uint16, device="cuda")
    with pytest.raises(ValueError):
        ops.resize_u10(x, (9, 13), out=torch.zeros(2 * 9 * 13 * 3 + 1, dtype=torch.uint16, device="cuda"))
    for bad in [(3, 13), (9, 49), (33, 24), (0, 0)]:
        with pytest.raises(ValueError):
            ops.resize_u10(x, bad)
    with pytest.raises(ValueError):
        ops.resize_u10(torch.zeros((2, 16, 24, 2), dtype=torch.uint16, device="cuda"), (9, 13))
    with pytest.raises(TypeError):
        ops.resize_u10(x.view(torch.int16), (9, 13))
    with pytest.raises(TypeError):
        ops.resize_u10(torch.zeros((2, 16, 24, 3), dtype=torch.uint8, device="cuda"), (9, 13))
    with pytest.raises(TypeError):
        ops.resize_u10(x.cpu(), (9, 13))


# ---- 4. the session ---------------------------------------------------------------------------------------------------------------------
def _engine_with(geom, w, precision="fp32"):
    e = PFNLEngine(geom, device=0)
    e.load_weights(w)
    if precision != "fp32":
        e.set_option("precision", precision)
    return e


def _stream_all(vs, frames, device=False, dtype=torch.uint16):
    """push one frame at a time, pop after every push, then end: [(index, frame)] in delivery order, frames as numpy"""
    got = []
    for f in frames:
        got += vs.push(torch.from_numpy(f).cuda() if device else f)
        got += vs.pop_ready()
    got += vs.end()
    if device:
        assert all(torch.is_tensor(f) and f.is_cuda and f.dtype == dtype for _, f in got)
        got = [(i, _host16(f) if dtype == torch.uint16 else f.cpu().numpy()) for i, f in got]
    else:
        assert all(isinstance(f, np.ndarray) and f.dtype == (np.uint16 if dtype == torch.uint16 else np.uint8) for _, f in got)
    return got


def _explicit_fp32(eng, frames_u8, batch, T):
    """the session's batches through the single ops on `eng`: the fp32 result on the host, [F,sH,sW,3]"""
    F = frames_u8.shape[0]
    dev = torch.from_numpy((frames_u8 / 255.).astype(np.float32)).cuda()
    outs = []
    for first in range(0, F, batch):
        count = min(batch, F - first)
        outs.append(eng.forward(ops.gather_windows(dev, first, count, T))[:, 0].cpu().numpy())
    sr = np.concatenate(outs)
    assert sr.dtype == np.float32
    return sr


def _expected(q10, fmt, size, matrix, full):
    rgb = q10 if size is None else np.stack([depth10.resize10(f, *size) for f in q10])
    return rgb if fmt == "rgb10" else np.stack([depth10.from_rgb10(f, fmt, matrix, full) for f in rgb])


SESSIONS = [(9, 4, 16, 24, 1, [(36, 54), (96, 160)], "fp32"), (5, 3, 16, 24, 1, [(36, 54), (96, 160)], "fp32"),
            (2, 5, 16, 24, 1, [(36, 54), (96, 160)], "fp32"), (6, 2, 64, 64, 2, [(144, 144)], "fp32"), (9, 4, 16, 24, 1, [(36, 54), (96, 160)], "bf16")]


@pytest.mark.parametrize("F,batch,H,W,nb,sizes,precision", SESSIONS)
def test_session_equals_the_explicit_path_sample_for_sample(F, batch, H, W, nb, sizes, precision):
    """What a session with a 10-bit output format delivers = per batch quantise10 of the forward of the gathered windows on a second engine,
    then resize10, then from_rgb10 - the host functions on the fp32 result; host frames and device tensors; the format survives reset;
    the plain session and the options are afterwards what they were."""
    geom = PFNLGeometry(num_block=nb)
    w = synth.synthetic_weights(geom, seed=0)
    eng, eng2 = _engine_with(geom, w, precision), _engine_with(geom, w, precision)
    before = {k: eng.get_option(k) for k in eng.OPTION_KEYS}
    lr = np.random.default_rng(F * 10 + batch).integers(0, 256, (F, H, W, 3), np.uint8)
    matrix, full = ("bt709", False) if nb == 1 else ("bt601", True)
    with eng.open_stream(H, W, batch) as vs:
        plain = np.stack([f for _, f in _stream_all(vs, list(lr), dtype=torch.uint8)])
    q10 = depth10.quantise10(_explicit_fp32(eng2, lr, batch, geom.num_frames))
    assert q10.shape == (F, 4 * H, 4 * W, 3) and len(np.unique(q10)) > 64       # (frames with content)
    for size in [None] + sizes:
        oH, oW = size if size is not None else (4 * H, 4 * W)
        for fmt in ("rgb10", "p010", "i010"):
            want = _expected(q10, fmt, size, matrix, full)
            with eng.open_stream(H, W, batch, out_format=fmt, out_size=size, matrix=matrix, full_range=full) as vs:
                assert (vs.pixel_format, vs.out_format, vs.out_size) == ("rgb24", fmt, size)
                for device in (False, True):
                    got = _stream_all(vs, list(lr), device)
                    assert [i for i, _ in got] == list(range(F))
                    sr = np.stack([f for _, f in got])
                    assert sr.dtype == np.uint16 and sr.shape == want.shape == ((F, oH, oW, 3) if fmt == "rgb10" else (F, oH * 3 // 2, oW))
                    assert np.array_equal(sr, want), (fmt, device, size, int((sr != want).sum()))
                    vs.reset()                                                  # the format and the size survive
    assert {k: eng.get_option(k) for k in eng.OPTION_KEYS} == before
    with eng.open_stream(H, W, batch) as vs:                                    # and the plain session is what it was
        assert np.array_equal(np.stack([f for _, f in _stream_all(vs, list(lr), dtype=torch.uint8)]), plain)
    eng.close()
    eng2.close()


def test_nv12_in_p010_out_and_the_same_picture_as_at_8_bits():
    F, batch, H, W = 7, 3, 16, 24
    geom = PFNLGeometry(num_block=1)
    w = synth.synthetic_weights(geom, seed=0)
    eng, eng2 = _engine_with(geom, w), _engine_with(geom, w)
    rng = np.random.default_rng(31)
    nv12 = [yuv.pack(rng.integers(0, 256, (H, W), np.uint8), rng.integers(0, 256, (H // 2, W // 2), np.uint8),
                     rng.integers(0, 256, (H // 2, W // 2), np.uint8), "nv12") for _ in range(F)]
    rgb_in = np.stack([yuv.to_rgb(f, "nv12", H, W, "bt601", False) for f in nv12])
    q10 = depth10.quantise10(_explicit_fp32(eng2, rgb_in, batch, geom.num_frames))
    want = _expected(q10, "p010", (36, 54), "bt601", False)
    with eng.open_stream(H, W, batch, pixel_format="nv12", out_format="p010", matrix="bt601", out_size=(36, 54)) as vs:
        assert (vs.pixel_format, vs.out_format) == ("nv12", "p010")
        for device in (False, True):
            got = np.stack([f for _, f in _stream_all(vs, [f.reshape(-1) for f in nv12] if not device else nv12, device)])
            assert got.shape == (F, 54, 54) and np.array_equal(got, want)
            vs.reset()
    # 5. the same picture: RGB10 and the plain session's bytes round the same fp32 value, one to 1023 levels and one to 255
    with eng.open_stream(H, W, batch) as vs:
        v8 = np.stack([f for _, f in _stream_all(vs, list(rgb_in), dtype=torch.uint8)]).astype(np.int64)
    with eng.open_stream(H, W, batch, out_format="rgb10") as vs:
        v10 = np.stack([f for _, f in _stream_all(vs, list(rgb_in))]).astype(np.int64)
    assert np.array_equal(v10, q10)
    # |v10 / 1023 - v8 / 255| <= 0.5 / 1023 + 0.5 / 255, over the common denominator 2 * 1023 * 255
    worst = int(np.abs(2 * (255 * v10 - 1023 * v8)).max())
    print("max |v10 / 1023 - v8 / 255| = %.6f, bound %.6f" % (worst / (2 * 1023 * 255), (255 + 1023) / (2 * 1023 * 255)))
    assert worst <= 255 + 1023
    assert len(np.unique(v10)) > len(np.unique(v8))                             # (and it resolves more levels)
    eng.close()
    eng2.close()


# ---- 6. the range fence -----------------------------------------------------------------------------------------------------------------
def test_recomputed_batches_leave_at_10_bits():
    """The setup of tests/test_gpu_stream.py test_session_recomputes_out_of_range_batches (conv0 x 4e5 leaves binary16's range, convmerge2
    x 1e-6 brings the result back onto the scale of the samples): every batch is delivered from the strict kernels' result."""
    lr_u8 = np.random.default_rng(21).integers(0, 256, size=(7, 12, 20, 3), dtype=np.uint8)
    geom = PFNLGeometry(num_block=1)
    w = synth.synthetic_weights(geom, seed=1)
    w["nlvsr/conv0/kernel"] = (w["nlvsr/conv0/kernel"] * 4e5).astype(np.float32)
    w["nlvsr/convmerge2/kernel"] = (w["nlvsr/convmerge2/kernel"] * 1e-6).astype(np.float32)
    eng = _engine_with(geom, w)
    with eng.open_stream(12, 20, 3, out_format="p010") as vs:
        got = _stream_all(vs, list(lr_u8))
        assert eng.get_option("strict_fp32") == "off"                           # end + the last pop have put it back
    strict = _engine_with(geom, w)
    strict.set_option("strict_fp32", "on")
    sr = strict.forward(np.ascontiguousarray(M.sliding_windows((lr_u8 / 255.).astype(np.float32), 7)))
    assert np.isfinite(sr).all()
    want = np.stack([depth10.from_rgb10(f, "p010") for f in depth10.quantise10(sr[:, 0])])
    assert [i for i, _ in got] == list(range(7))
    assert np.array_equal(np.stack([f for _, f in got]), want)
    assert len(np.unique(want)) > 16                                            # (frames with content, not a flat failure value)
    assert eng.range_flagged() is False
    eng.close()
    strict.close()


# ---- 7. refusals on a live session ------------------------------------------------------------------------------------------------------
def test_state_and_validation():
    H, W, batch = 16, 24, 2                                                     # the network delivers 64 x 96
    geom = PFNLGeometry(num_block=1)
    eng = _engine_with(geom, synth.synthetic_weights(geom, seed=0))
    lib = eng._lib
    lr = list(np.random.default_rng(61).integers(0, 256, (6, H, W, 3), np.uint8))
    with eng.open_stream(H, W, batch, out_format="p010") as vs:
        first = _stream_all(vs, lr)
        assert first[0][1].shape == (96, 96)
        vs.reset()
        for in_fmt in (3, 4, 5):                                                # 10-bit input is not built
            assert lib.pfnl_stream_format(vs._s, in_fmt, 4, 1, 0) == -1 and b"10-bit input" in lib.pfnl_last_error()
        assert lib.pfnl_stream_format(vs._s, 0, 6, 1, 0) == -1 and lib.pfnl_stream_format(vs._s, 0, 4, 2, 0) == -1
        assert lib.pfnl_stream_format(vs._s, 1, 3, 1, 0) == -1 and b"RGB10" in lib.pfnl_last_error()   # RGB10 goes with RGB input
        vs.push(lr[0])
        for fmts in ((0, 5), (0, 0), (0, 3), (1, 4)):                           # a change after the first frame: PFNL_ERR_STATE ...
            assert lib.pfnl_stream_format(vs._s, *fmts, 1, 0) == -2 and b"before the first frame" in lib.pfnl_last_error(), fmts
        assert lib.pfnl_stream_format(vs._s, 4, 4, 1, 0) == -1                  # (a bad format is a bad format at any time)
        got = vs.pop_ready()                                                    # ... and nothing changed: the sequence carries on as P010
        for f in lr[1:]:
            got += vs.push(f)
            got += vs.pop_ready()
        got += vs.end()
        assert [i for i, _ in got] == [i for i, _ in first] == list(range(6))
        assert np.array_equal(np.stack([f for _, f in got]), np.stack([f for _, f in first]))
        vs.reset()
        # an odd output size and I010, whichever call comes second; RGB10 takes it
        assert lib.pfnl_stream_resize(vs._s, 37, 54) == -1 and b"even" in lib.pfnl_last_error()        # (the session is P010)
        assert lib.pfnl_stream_format(vs._s, 0, 3, 1, 0) == 0 and lib.pfnl_stream_resize(vs._s, 37, 54) == 0
        assert lib.pfnl_stream_format(vs._s, 0, 5, 1, 0) == -1 and b"even" in lib.pfnl_last_error()
        assert lib.pfnl_stream_resize(vs._s, 36, 54) == 0 and lib.pfnl_stream_format(vs._s, 0, 5, 1, 0) == 0
        assert lib.pfnl_stream_resize(vs._s, 36, 55) == -1 and b"even" in lib.pfnl_last_error()
        vs.out_format, vs.out_size = "i010", (36, 54)                           # (the raw calls went past the Python object)
        i010 = np.stack([f for _, f in _stream_all(vs, lr)])                    # the refused calls changed nothing: 36 x 54, I010
        p010_full = np.stack([f for _, f in first])
        rgb = None
        vs.reset()
        assert lib.pfnl_stream_resize(vs._s, 0, 0) == 0                         # the network's size again, still I010: P010's values
        vs.out_size = None
        full = np.stack([f for _, f in _stream_all(vs, lr)])
        for a, b in zip(full, p010_full):
            for pa, pb in zip(depth10.planes10(a, "i010", 64, 96), depth10.planes10(b, "p010", 64, 96)):
                assert np.array_equal(pa, pb)
        vs.reset()
        assert lib.pfnl_stream_format(vs._s, 0, 3, 1, 0) == 0 and lib.pfnl_stream_resize(vs._s, 36, 54) == 0
        vs.out_format, vs.out_size = "rgb10", (36, 54)
        rgb = np.stack([f for _, f in _stream_all(vs, lr)])
        assert rgb.shape == (6, 36, 54, 3)
        assert np.array_equal(i010, np.stack([depth10.from_rgb10(f, "i010") for f in rgb]))
    for kw in ({"pixel_format": "p010"}, {"out_format": "i010", "out_size": (37, 54)}, {"out_format": "p010", "out_size": (36, 55)},
               {"pixel_format": "i420", "out_format": "rgb10"}):
        with pytest.raises(ValueError):
            eng.open_stream(H, W, batch, **kw)
    with eng.open_stream(H, W, batch, out_format="rgb10", out_size=(37, 55)) as vs:   # (nothing was left open by the refusals; odd sizes are fine as RGB)
        odd = np.stack([f for _, f in _stream_all(vs, lr)])
    assert odd.shape == (6, 37, 55, 3) and odd.dtype == np.uint16 and int(odd.max()) <= 1023
    eng.close()


ROUTE_WALK = [("rgb24", None), ("p010", (36, 54)), ("nv12", (36, 54)), ("i010", None), ("rgb10", (37, 55)), ("i420", (96, 160)), ("rgb24", None)]


def test_one_session_walks_every_route():
    """One open session through seven settings with a reset between them - each makes the slot table grow, shrink or free another stage
    (pfnl_amd/csrc/capi_stream.hip apply_setting) - delivers at every step the bytes of a fresh session opened with that setting, through
    host pointers and through device pointers.  Two batches per sequence, the second partial."""
    from pfnl_amd import _capi
    H, W, batch = 16, 24, 2
    geom = PFNLGeometry(num_block=1)
    eng = _engine_with(geom, synth.synthetic_weights(geom, seed=0))
    lib = eng._lib
    lr = list(np.random.default_rng(71).integers(0, 256, (5, H, W, 3), np.uint8))
    dtype = lambda fmt: torch.uint16 if fmt in _capi.TEN_BIT_FORMATS else torch.uint8   # noqa: E731
    fresh = {}
    for fmt, size in dict.fromkeys(ROUTE_WALK):
        with eng.open_stream(H, W, batch, out_format=fmt, out_size=size) as vs:
            fresh[fmt, size] = np.stack([f for _, f in _stream_all(vs, lr, dtype=dtype(fmt))])
    assert len(fresh) == 6 and len({f.tobytes() for f in fresh.values()}) == 6
    walked = []
    with eng.open_stream(H, W, batch) as vs:
        for fmt, size in ROUTE_WALK:
            calls = [lambda: lib.pfnl_stream_format(vs._s, 0, _capi.PIXEL_FORMATS[fmt], 1, 0), lambda: lib.pfnl_stream_resize(vs._s, *(size or (0, 0)))]
            for call in (reversed(calls) if fmt in _capi.FORMATS_420 else calls):   # a 4:2:0 format comes behind its even size, an odd size behind RGB
                assert call() == 0, (fmt, size, lib.pfnl_last_error())
            vs.out_format, vs.out_size = fmt, size                                  # (the raw calls went past the Python object)
            for device in (False, True):
                got = _stream_all(vs, lr, device, dtype(fmt))
                assert [i for i, _ in got] == list(range(5))
                sr = np.stack([f for _, f in got])
                want = fresh[fmt, size]
                assert sr.dtype == want.dtype and sr.shape == want.shape and np.array_equal(sr, want), (fmt, size, device)
                vs.reset()
            walked.append(sr)
    assert np.array_equal(walked[6], walked[0])
    eng.close()
