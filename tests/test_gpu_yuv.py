"""YUV 4:2:0 on a real MI355X (include/pfnl_hip.h pfnl_stream_format; pfnl_amd/csrc/yuv.hip): both kernels and the session's two edges
against the host rule pfnl_amd/yuv.py, byte for byte - no tolerance anywhere."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfnl_amd import ops, scene, synth, yuv  # noqa: E402
from pfnl_amd.engine import PFNLEngine  # noqa: E402
from pfnl_amd.spec import PFNLGeometry  # noqa: E402

PAIRS = [("bt601", False), ("bt601", True), ("bt709", False), ("bt709", True)]
# (2, 2), (2, 6), (6, 2): nothing but edges; (18, 34), (34, 66): single bytes, W / 2 odd; (10, 36): 4-byte words; (16, 64): 16-byte words
SHAPES = [(2, 2), (2, 6), (6, 2), (18, 34), (10, 36), (16, 64), (34, 66)]


def _bytes_with_all_values(rng, shape):
    a = rng.integers(0, 256, size=shape, dtype=np.uint8)
    flat = a.reshape(-1)
    if flat.size >= 256:
        flat[rng.permutation(flat.size)[:256]] = np.arange(256, dtype=np.uint8)
        assert len(np.unique(flat)) == 256
    return a


def _extreme_blocks(rng, shape, block=2):
    """0 or 255 in blocks of `block` samples: every clip of either direction fires next to its opposite"""
    small = rng.integers(0, 2, size=tuple((s + block - 1) // block for s in shape[:2]) + tuple(shape[2:]), dtype=np.uint8) * 255
    return np.repeat(np.repeat(small, block, axis=0), block, axis=1)[:shape[0], :shape[1]]


def _yuv_frames(n, H, W, fmt, seed):
    """n packed frames: random bytes with every value present, the last of several made of extreme planes"""
    rng = np.random.default_rng(seed)
    frames = [_bytes_with_all_values(rng, (H * 3 // 2, W)) for _ in range(n)]
    if n > 1:
        frames[-1] = yuv.pack(_extreme_blocks(rng, (H, W)), _extreme_blocks(rng, (H // 2, W // 2)), _extreme_blocks(rng, (H // 2, W // 2)), fmt)
    return np.stack(frames)


def _rgb_frames(n, H, W, seed):
    rng = np.random.default_rng(seed)
    frames = [_bytes_with_all_values(rng, (H, W, 3)) for _ in range(n)]
    if n > 1:
        frames[-1] = _extreme_blocks(rng, (H, W, 3))
    return np.stack(frames)


# ---- 1. the two ops -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", yuv.FORMATS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_yuv420_to_rgb_equals_the_host_rule(H, W, fmt):
    for n in (1, 3):
        frames = _yuv_frames(n, H, W, fmt, seed=H * 1000 + W + n)
        dev = torch.from_numpy(frames).cuda()
        for matrix, full in PAIRS:
            got = ops.yuv420_to_rgb(dev, fmt, H, W, matrix, full).cpu().numpy()
            want = np.stack([yuv.to_rgb(f, fmt, H, W, matrix, full) for f in frames])
            assert got.dtype == np.uint8 and got.shape == want.shape == (n, H, W, 3)
            assert np.array_equal(got, want), (H, W, fmt, n, matrix, full, int((got != want).sum()))
            if n > 1 and H * W >= 256:
                assert want[-1].min() == 0 and want[-1].max() == 255           # the extreme planes clip at both ends


@pytest.mark.parametrize("fmt", yuv.FORMATS)
@pytest.mark.parametrize("H,W", SHAPES)
def test_rgb_to_yuv420_equals_the_host_rule(H, W, fmt):
    for n in (1, 3):
        frames = _rgb_frames(n, H, W, seed=H * 1000 + W + 10 + n)
        dev = torch.from_numpy(frames).cuda()
        for matrix, full in PAIRS:
            got = ops.rgb_to_yuv420(dev, fmt, matrix, full).cpu().numpy()
            want = np.stack([yuv.from_rgb(f, fmt, matrix, full) for f in frames])
            assert got.dtype == np.uint8 and got.shape == want.shape == (n, H * 3 // 2, W)
            assert np.array_equal(got, want), (H, W, fmt, n, matrix, full, int((got != want).sum()))


@pytest.mark.parametrize("fmt", yuv.FORMATS)
@pytest.mark.parametrize("H,W", [(16, 64), (10, 36)])          # shapes whose aligned form uses words: at an odd address it must not
def test_unaligned_pointers_take_the_byte_form_and_stay_inside_the_destination(H, W, fmt):
    n, slack = 2, 64
    pattern = lambda size: (np.arange(size) * 7 + 3).astype(np.uint8)           # noqa: E731
    yb, rb = n * H * W * 3 // 2, n * H * W * 3
    frames = _yuv_frames(n, H, W, fmt, seed=5)
    rgbs = _rgb_frames(n, H, W, seed=6)
    for off in (1, 4):                                                          # single bytes; 4-byte words at most
        src = torch.zeros(off + yb, dtype=torch.uint8, device="cuda")
        src[off:] = torch.from_numpy(frames.reshape(-1)).cuda()
        dst = torch.from_numpy(pattern(off + rb + slack)).cuda()
        ops.yuv420_to_rgb(src[off:], fmt, H, W, "bt601", False, out=dst[off:off + rb])
        got = dst.cpu().numpy()
        want = np.stack([yuv.to_rgb(f, fmt, H, W, "bt601", False) for f in frames])
        assert np.array_equal(got[off:off + rb].reshape(want.shape), want)
        assert np.array_equal(got[:off], pattern(off + rb + slack)[:off]) and np.array_equal(got[off + rb:], pattern(off + rb + slack)[off + rb:])
        src = torch.zeros(off + rb, dtype=torch.uint8, device="cuda")
        src[off:] = torch.from_numpy(rgbs.reshape(-1)).cuda()
        dst = torch.from_numpy(pattern(off + yb + slack)).cuda()
        ops.rgb_to_yuv420(src[off:].view(n, H, W, 3), fmt, "bt601", False, out=dst[off:off + yb])
        got = dst.cpu().numpy()
        want = np.stack([yuv.from_rgb(f, fmt, "bt601", False) for f in rgbs])
        assert np.array_equal(got[off:off + yb].reshape(want.shape), want)
        assert np.array_equal(got[:off], pattern(off + yb + slack)[:off]) and np.array_equal(got[off + yb:], pattern(off + yb + slack)[off + yb:])


# ---- 2. the session -------------------------------------------------------------------------------------------------------------------
def _engine_with(geom, w, precision="fp32"):
    e = PFNLEngine(geom, device=0)
    e.load_weights(w)
    if precision != "fp32":
        e.set_option("precision", precision)
    return e


def _stream_all(vs, frames, device=False):
    """push one frame at a time, pop after every push, then end: [(index, frame)] in delivery order, frames as numpy"""
    got = []
    for f in frames:
        got += vs.push(torch.from_numpy(f).cuda() if device else f)
        got += vs.pop_ready()
    got += vs.end()
    if device:
        assert all(torch.is_tensor(f) and f.is_cuda and f.dtype == torch.uint8 for _, f in got)
        got = [(i, f.cpu().numpy()) for i, f in got]
    return got


def _planes_of_sequence(F, H, W, seed):
    rng = np.random.default_rng(seed)
    return [(rng.integers(0, 256, (H, W), np.uint8), rng.integers(0, 256, (H // 2, W // 2), np.uint8), rng.integers(0, 256, (H // 2, W // 2), np.uint8))
            for _ in range(F)]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("F,batch,H,W,nb", [(9, 4, 16, 24, 1), (5, 3, 16, 24, 1), (2, 5, 16, 24, 1), (6, 2, 64, 64, 2)])
def test_yuv_session_equals_the_rgb_session_converted_on_the_host(F, batch, H, W, nb, precision):
    """What a YUV session delivers = from_rgb of what a plain RGB session on a second engine delivers for to_rgb of the same frames; NV12 and
    I420 hold the same planes, so one RGB run serves both; host frames and device tensors."""
    geom = PFNLGeometry(num_block=nb)
    w = synth.synthetic_weights(geom, seed=0)
    eng, eng2 = _engine_with(geom, w, precision), _engine_with(geom, w, precision)
    before = {k: eng.get_option(k) for k in eng.OPTION_KEYS}
    planes = _planes_of_sequence(F, H, W, seed=F * 10 + batch)
    matrix, full = ("bt709", False) if nb == 1 else ("bt601", True)
    rgb_in = [yuv.to_rgb(yuv.pack(*p, "nv12"), "nv12", H, W, matrix, full) for p in planes]
    with eng2.open_stream(H, W, batch) as vs:
        rgb_sr = _stream_all(vs, rgb_in)
    assert [i for i, _ in rgb_sr] == list(range(F))
    for fmt in yuv.FORMATS:
        frames = [yuv.pack(*p, fmt) for p in planes]
        want = np.stack([yuv.from_rgb(f, fmt, matrix, full) for _, f in rgb_sr])
        with eng.open_stream(H, W, batch, pixel_format=fmt, matrix=matrix, full_range=full) as vs:
            assert (vs.pixel_format, vs.out_format, vs.matrix, vs.full_range) == (fmt, fmt, matrix, full)
            for device in (False, True):
                got = _stream_all(vs, frames, device)
                assert [i for i, _ in got] == list(range(F))
                sr = np.stack([f for _, f in got])
                assert sr.dtype == np.uint8 and sr.shape == want.shape == (F, 4 * H * 3 // 2, 4 * W)
                assert np.array_equal(sr, want), (fmt, device, int((sr != want).sum()))
                vs.reset()                                                      # the format survives
    assert {k: eng.get_option(k) for k in eng.OPTION_KEYS} == before
    eng.close()
    eng2.close()


def test_mixed_formats_and_flat_frames():
    F, batch, H, W = 7, 3, 16, 24
    geom = PFNLGeometry(num_block=1)
    w = synth.synthetic_weights(geom, seed=0)
    eng, eng2 = _engine_with(geom, w), _engine_with(geom, w)
    planes = _planes_of_sequence(F, H, W, seed=31)
    nv12 = [yuv.pack(*p, "nv12") for p in planes]
    rgb_in = [yuv.to_rgb(f, "nv12", H, W, "bt601", False) for f in nv12]
    with eng2.open_stream(H, W, batch) as vs:
        rgb_of_nv12 = np.stack([f for _, f in _stream_all(vs, rgb_in)])
    rgb_frames = list(np.random.default_rng(32).integers(0, 256, (F, H, W, 3), np.uint8))
    with eng2.open_stream(H, W, batch) as vs:
        rgb_of_rgb = np.stack([f for _, f in _stream_all(vs, rgb_frames)])
    with eng.open_stream(H, W, batch, pixel_format="nv12", out_format="rgb24", matrix="bt601") as vs:      # NV12 in, RGB out
        assert (vs.pixel_format, vs.out_format) == ("nv12", "rgb24")
        got = np.stack([f for _, f in _stream_all(vs, [f.reshape(-1) for f in nv12])])                     # flat frames are frames too
        assert got.shape == (F, 4 * H, 4 * W, 3) and np.array_equal(got, rgb_of_nv12)
        vs.reset()
        got = np.stack([f for _, f in _stream_all(vs, nv12, device=True)])
        assert np.array_equal(got, rgb_of_nv12)
    with eng.open_stream(H, W, batch, out_format="i420", matrix="bt601") as vs:                            # RGB in, I420 out
        assert (vs.pixel_format, vs.out_format) == ("rgb24", "i420")
        want = np.stack([yuv.from_rgb(f, "i420", "bt601", False) for f in rgb_of_rgb])
        for device in (False, True):
            got = np.stack([f for _, f in _stream_all(vs, rgb_frames, device)])
            assert got.shape == (F, 4 * H * 3 // 2, 4 * W) and np.array_equal(got, want)
            vs.reset()
    with eng.open_stream(H, W, batch) as vs:                                                               # and the plain session is what it was
        assert np.array_equal(np.stack([f for _, f in _stream_all(vs, rgb_frames)]), rgb_of_rgb)
    eng.close()
    eng2.close()


def test_scene_detector_sees_the_converted_frames():
    """NV12 in, two synthetic scenes: cuts and every frame's (scene_first, sad) equal those of an RGB session fed to_rgb of the frames, and
    the host rule on those RGB frames."""
    H, W, batch = 16, 24, 3
    rng = np.random.default_rng(41)
    lengths, levels = (5, 6), (60, 190)                                         # two scenes around different luma levels, chroma alike
    nv12 = []
    for length, level in zip(lengths, levels):
        base = np.clip(level + rng.integers(-20, 21, (H, W)), 0, 255)
        for _ in range(length):
            Y = np.clip(base + rng.integers(-3, 4, (H, W)), 0, 255).astype(np.uint8)
            nv12.append(yuv.pack(Y, rng.integers(118, 139, (H // 2, W // 2), np.uint8), rng.integers(118, 139, (H // 2, W // 2), np.uint8), "nv12"))
    rgb = [yuv.to_rgb(f, "nv12", H, W) for f in nv12]
    sf = scene.scene_first(rgb, threshold=10.0)
    assert list(sf) == [0] * 5 + [5] * 6                                        # the host rule finds the one placed cut
    sads = scene.frame_sads(rgb)
    geom = PFNLGeometry(num_block=1)
    w = synth.synthetic_weights(geom, seed=0)
    eng, eng2 = _engine_with(geom, w), _engine_with(geom, w)

    def run(e, frames, device, **kw):
        with e.open_stream(H, W, batch, scene_cut=10.0, **kw) as vs:
            out, infos = [], []
            for f in frames:
                assert vs.push(torch.from_numpy(f).cuda() if device else f) == []   # (everything deliverable was popped before)
                while vs.ready():
                    out.append(vs.pop())
                    infos.append(vs.last_info)
            vs._lib.pfnl_stream_end(vs._handle())
            while vs.ready():
                out.append(vs.pop())
                infos.append(vs.last_info)
            frames_out = [f.cpu().numpy() if torch.is_tensor(f) else f for _, f in out]
            return [i for i, _ in out], frames_out, infos, list(vs.cuts)

    idx_r, sr_r, infos_r, cuts_r = run(eng2, rgb, False)
    assert idx_r == list(range(11)) and cuts_r == [5]
    assert infos_r == [(int(sf[k]), int(sads[k])) for k in range(11)]
    for device in (False, True):
        idx, sr, infos, cuts = run(eng, nv12, device, pixel_format="nv12", out_format="rgb24")
        assert idx == idx_r and cuts == cuts_r and infos == infos_r
        assert np.array_equal(np.stack(sr), np.stack(sr_r))
    eng.close()
    eng2.close()


def test_reset_state_and_wrong_sized_frames():
    H, W, batch = 16, 24, 2
    geom = PFNLGeometry(num_block=1)
    eng = _engine_with(geom, synth.synthetic_weights(geom, seed=0))
    lib = eng._lib
    planes = _planes_of_sequence(6, H, W, seed=51)
    i420 = [yuv.pack(*p, "i420") for p in planes]
    with eng.open_stream(H, W, batch, pixel_format="i420") as vs:
        first = _stream_all(vs, i420)
        vs.reset()
        assert (vs.pixel_format, vs.out_format) == ("i420", "i420")
        vs.push(i420[0])
        assert lib.pfnl_stream_format(vs._s, 0, 0, 1, 0) == -2 and b"before the first frame" in lib.pfnl_last_error()   # PFNL_ERR_STATE ...
        assert lib.pfnl_stream_format(vs._s, 1, 3, 1, 0) == -1 and lib.pfnl_stream_format(vs._s, 1, 1, 5, 0) == -1
        for bad in (np.zeros((H, W, 3), np.uint8), np.zeros((H * 3 // 2, W + 2), np.uint8), np.zeros((H * W * 3 // 2 - 1,), np.uint8),
                    np.zeros((H * 3 // 2, W), np.int8), torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")):
            with pytest.raises(ValueError):
                vs.push(bad)
        got = vs.pop_ready()                                                    # ... and nothing changed: the sequence carries on, still I420
        for f in i420[1:]:
            got += vs.push(f)
            got += vs.pop_ready()
        got += vs.end()
        assert [i for i, _ in got] == [i for i, _ in first] == list(range(6))
        assert np.array_equal(np.stack([f for _, f in got]), np.stack([f for _, f in first]))
        vs.reset()
        assert lib.pfnl_stream_format(vs._s, 0, 0, 1, 0) == 0                   # before a first frame: back to the default
        vs.pixel_format = vs.out_format = "rgb24"                               # (the raw call went past the Python object)
        rgb = list(np.random.default_rng(52).integers(0, 256, (3, H, W, 3), np.uint8))
        plain = _stream_all(vs, rgb)
    with eng.open_stream(H, W, batch) as vs:
        want = _stream_all(vs, rgb)
    assert np.array_equal(np.stack([f for _, f in plain]), np.stack([f for _, f in want]))
    eng.close()


def test_recomputed_batches_leave_in_the_output_format():
    """The range fence (tests/test_gpu_stream.py test_session_recomputes_out_of_range_batches: conv0 x 4e5 leaves binary16's range, convmerge2
    x 1e-6 brings the result back to bytes): the batches the session computes again on the strict kernels are converted like any other."""
    H, W, batch = 12, 20, 3
    lr_u8 = np.random.default_rng(21).integers(0, 256, size=(7, H, W, 3), dtype=np.uint8)
    geom = PFNLGeometry(num_block=1)
    w = synth.synthetic_weights(geom, seed=1)
    w["nlvsr/conv0/kernel"] = (w["nlvsr/conv0/kernel"] * 4e5).astype(np.float32)
    w["nlvsr/convmerge2/kernel"] = (w["nlvsr/convmerge2/kernel"] * 1e-6).astype(np.float32)
    eng, eng2 = _engine_with(geom, w), _engine_with(geom, w)
    with eng2.open_stream(H, W, batch) as vs:
        rgb_sr = _stream_all(vs, list(lr_u8))
    assert eng2.range_flagged() is False and len(rgb_sr) == 7
    with eng.open_stream(H, W, batch, out_format="nv12") as vs:
        got = _stream_all(vs, list(lr_u8))
        assert eng.get_option("strict_fp32") == "off"                           # end + the last pop have put it back
    assert [i for i, _ in got] == list(range(7))
    want = np.stack([yuv.from_rgb(f, "nv12") for _, f in rgb_sr])
    assert np.array_equal(np.stack([f for _, f in got]), want)
    assert len(np.unique(want)) > 16                                            # (frames with content, not a flat failure value)
    eng.close()
    eng2.close()
