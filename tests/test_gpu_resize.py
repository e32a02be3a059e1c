"""The output size of the streaming session on a real MI355X (include/pfnl_hip.h pfnl_stream_resize; pfnl_amd/csrc/resize.hip): the kernel
and the session against the host rule pfnl_amd/resize.py, byte for byte - no tolerance anywhere."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfnl_amd import ops, resize, synth, yuv  # noqa: E402
from pfnl_amd.engine import PFNLEngine  # noqa: E402
from pfnl_amd.spec import PFNLGeometry  # noqa: E402

# (8, 8) -> (2, 2): every tap clamped; (16, 24) twice: the identity; (64, 96) -> (16, 24): 16 taps; -> (128, 192): 16-byte stores, two tiles
# across and eight down; (20, 600) -> (10, 333): six tiles across, an odd width; the others: ratios that are no integers, both directions
GEOMETRIES = [((8, 8), (2, 2)), ((16, 24), (16, 24)), ((16, 24), (9, 13)), ((64, 96), (36, 54)), ((64, 96), (16, 24)), ((64, 96), (128, 192)),
              ((48, 80), (90, 100)), ((40, 200), (30, 75)), ((20, 600), (10, 333))]


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


def _rgb_frames(n, H, W, seed):
    """n frames of random bytes with every value present; the last one 0 / 255 blocks of 2 x 2"""
    rng = np.random.default_rng(seed)
    frames = [_bytes_with_all_values(rng, (H, W, 3)) for _ in range(n)]
    frames[-1] = _extreme_blocks(rng, (H, W, 3))
    return np.stack(frames)


# ---- 1. the op --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,out", GEOMETRIES)
def test_resize_equals_the_host_rule(size, out):
    (H, W), (oH, oW) = size, out
    for n in (1, 3):
        frames = _rgb_frames(n, H, W, seed=H * 1000 + W + n)
        want = np.stack([resize.resize(f, oH, oW) for f in frames])
        got = ops.resize_u8(torch.from_numpy(frames).cuda(), (oH, oW)).cpu().numpy()
        assert got.dtype == np.uint8 and got.shape == want.shape == (n, oH, oW, 3)
        assert np.array_equal(got, want), (size, out, n, int((got != want).sum()))
        if (H, W) != (oH, oW) and H * W >= 256:                                 # the block frame overshoots, and the clip removes it, at both ends
            raw = resize.resize_unclipped(frames[-1], oH, oW)
            assert raw.min() < 0 and raw.max() > 255
            assert want[-1].min() == 0 and want[-1].max() == 255
    single = ops.resize_u8(torch.from_numpy(frames[0]).cuda(), (oH, oW))          # [H,W,3] is a batch of one
    assert tuple(single.shape) == (1, oH, oW, 3) and np.array_equal(single.cpu().numpy()[0], want[0])


@pytest.mark.parametrize("size,out", [((64, 96), (128, 192)), ((40, 200), (30, 80)), ((16, 24), (9, 13))])   # two whose aligned form stores words
def test_unaligned_pointers_take_the_byte_form_and_stay_inside_the_destination(size, out):
    (H, W), (oH, oW) = size, out
    n, slack = 2, 64
    pattern = lambda count: (np.arange(count) * 7 + 3).astype(np.uint8)         # noqa: E731
    ib, ob = n * H * W * 3, n * oH * oW * 3
    frames = _rgb_frames(n, H, W, seed=7)
    want = np.stack([resize.resize(f, oH, oW) for f in frames])
    for off in (0, 1, 4):                                                       # (0 keeps slack + ob: the words end where the frames end)
        src = torch.zeros(off + ib, dtype=torch.uint8, device="cuda")
        src[off:] = torch.from_numpy(frames.reshape(-1)).cuda()
        guard = pattern(slack + off + ob + slack)
        dst = torch.from_numpy(guard).cuda()
        lo = slack + off
        ops.resize_u8(src[off:].view(n, H, W, 3), (oH, oW), out=dst[lo:lo + ob])
        got = dst.cpu().numpy()
        assert np.array_equal(got[lo:lo + ob].reshape(want.shape), want), (size, out, off)
        assert np.array_equal(got[:lo], guard[:lo]) and np.array_equal(got[lo + ob:], guard[lo + ob:]), (size, out, off)


def test_wrong_sizes_raise():
    x = torch.zeros((2, 16, 24, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        ops.resize_u8(x, (9, 13), out=torch.zeros(2 * 9 * 13 * 3 + 1, dtype=torch.uint8, device="cuda"))
    for bad in [(3, 13), (9, 49), (33, 24), (0, 0)]:
        with pytest.raises(ValueError):
            ops.resize_u8(x, bad)
    with pytest.raises(ValueError):
        ops.resize_u8(torch.zeros((2, 16, 24, 2), dtype=torch.uint8, device="cuda"), (9, 13))
    with pytest.raises(TypeError):
        ops.resize_u8(x.cpu(), (9, 13))


# ---- 2. the session ---------------------------------------------------------------------------------------------------------------------
def _engine_with(geom, w):
    e = PFNLEngine(geom, device=0)
    e.load_weights(w)
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


@pytest.mark.parametrize("F,batch,H,W,nb,sizes", [(9, 4, 16, 24, 1, [(36, 54), (96, 160)]), (5, 3, 16, 24, 1, [(36, 54), (96, 160)]),
                                                  (2, 5, 16, 24, 1, [(36, 54), (96, 160)]), (6, 2, 64, 64, 2, [(144, 144)])])
def test_resized_session_equals_the_plain_session_resized_on_the_host(F, batch, H, W, nb, sizes):
    """What a session with an output size delivers = resize.resize of what a plain session on a second engine delivers, and yuv.from_rgb of
    that in a YUV output format; host frames and device tensors; the setting survives reset."""
    geom = PFNLGeometry(num_block=nb)
    w = synth.synthetic_weights(geom, seed=0)
    eng, eng2 = _engine_with(geom, w), _engine_with(geom, w)
    before = {k: eng.get_option(k) for k in eng.OPTION_KEYS}
    lr = list(np.random.default_rng(F * 10 + batch).integers(0, 256, (F, H, W, 3), np.uint8))
    with eng2.open_stream(H, W, batch) as vs:
        assert vs.out_size is None
        plain = _stream_all(vs, lr)
    assert [i for i, _ in plain] == list(range(F)) and plain[0][1].shape == (4 * H, 4 * W, 3)
    for oH, oW in sizes:
        rgb = np.stack([resize.resize(f, oH, oW) for _, f in plain])
        assert len(np.unique(rgb)) > 16                                         # (frames with content)
        for fmt in ("rgb24", "nv12", "i420"):
            want = rgb if fmt == "rgb24" else np.stack([yuv.from_rgb(f, fmt) for f in rgb])
            with eng.open_stream(H, W, batch, out_format=fmt, out_size=(oH, oW)) as vs:
                assert vs.out_size == (oH, oW) and vs.out_format == fmt
                for device in (False, True):
                    got = _stream_all(vs, lr, device)
                    assert [i for i, _ in got] == list(range(F))
                    sr = np.stack([f for _, f in got])
                    assert sr.dtype == np.uint8 and sr.shape == want.shape == ((F, oH, oW, 3) if fmt == "rgb24" else (F, oH * 3 // 2, oW))
                    assert np.array_equal(sr, want), (fmt, device, (oH, oW), int((sr != want).sum()))
                    vs.reset()                                                  # the size survives
    assert {k: eng.get_option(k) for k in eng.OPTION_KEYS} == before
    with eng.open_stream(H, W, batch) as vs:                                    # and the plain session is what it was
        assert np.array_equal(np.stack([f for _, f in _stream_all(vs, lr)]), np.stack([f for _, f in plain]))
    eng.close()
    eng2.close()


def test_recomputed_batches_leave_resized():
    """The range fence (tests/test_gpu_yuv.py test_recomputed_batches_leave_in_the_output_format: conv0 x 4e5 leaves binary16's range,
    convmerge2 x 1e-6 brings the result back to bytes): the batches the session computes again on the strict kernels are resized - and
    converted - like any other."""
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
    want = np.stack([resize.resize(f, 30, 54) for _, f in rgb_sr])
    assert len(np.unique(want)) > 16                                            # (frames with content, not a flat failure value)
    for fmt in ("rgb24", "nv12"):
        with eng.open_stream(H, W, batch, out_format=fmt, out_size=(30, 54)) as vs:
            got = _stream_all(vs, list(lr_u8))
            assert eng.get_option("strict_fp32") == "off"                       # end + the last pop have put it back
        assert [i for i, _ in got] == list(range(7))
        expect = want if fmt == "rgb24" else np.stack([yuv.from_rgb(f, fmt) for f in want])
        assert np.array_equal(np.stack([f for _, f in got]), expect), fmt
    eng.close()
    eng2.close()


def test_state_and_validation():
    H, W, batch = 16, 24, 2                                                     # the network delivers 64 x 96
    geom = PFNLGeometry(num_block=1)
    eng = _engine_with(geom, synth.synthetic_weights(geom, seed=0))
    lib = eng._lib
    lr = list(np.random.default_rng(61).integers(0, 256, (6, H, W, 3), np.uint8))
    with eng.open_stream(H, W, batch) as vs:
        plain = _stream_all(vs, lr)
    with eng.open_stream(H, W, batch, out_size=(36, 54)) as vs:
        first = _stream_all(vs, lr)
        assert first[0][1].shape == (36, 54, 3)
        vs.reset()
        assert vs.out_size == (36, 54)
        vs.push(lr[0])
        assert lib.pfnl_stream_resize(vs._s, 0, 0) == -2 and b"before the first frame" in lib.pfnl_last_error()   # PFNL_ERR_STATE ...
        assert lib.pfnl_stream_resize(vs._s, 48, 48) == -2
        assert lib.pfnl_stream_resize(vs._s, 15, 54) == -1                      # (a bad size is a bad size at any time)
        got = vs.pop_ready()                                                    # ... and nothing changed: the sequence carries on at 36 x 54
        for f in lr[1:]:
            got += vs.push(f)
            got += vs.pop_ready()
        got += vs.end()
        assert [i for i, _ in got] == [i for i, _ in first] == list(range(6))
        assert np.array_equal(np.stack([f for _, f in got]), np.stack([f for _, f in first]))
        vs.reset()
        # outside the limits: below a quarter, above twice, above 16384, one of the two zero
        for bad in [(15, 54), (36, 23), (129, 54), (36, 193), (36, 20000), (0, 54), (36, 0), (-36, 54)]:
            assert lib.pfnl_stream_resize(vs._s, *bad) == -1 and b"resize" in lib.pfnl_last_error(), bad
        # a YUV output needs even sizes, whichever call comes second
        assert lib.pfnl_stream_resize(vs._s, 37, 54) == 0
        assert lib.pfnl_stream_format(vs._s, 0, 1, 1, 0) == -1 and b"even" in lib.pfnl_last_error()
        assert lib.pfnl_stream_resize(vs._s, 36, 54) == 0 and lib.pfnl_stream_format(vs._s, 0, 1, 1, 0) == 0
        assert lib.pfnl_stream_resize(vs._s, 36, 55) == -1 and b"even" in lib.pfnl_last_error()
        assert lib.pfnl_stream_resize(vs._s, 37, 54) == -1
        vs.out_format = "nv12"                                                  # (the raw calls went past the Python object)
        nv12 = _stream_all(vs, lr)                                              # the refused calls changed nothing: 36 x 54, NV12
        want = np.stack([yuv.from_rgb(resize.resize(f, 36, 54), "nv12") for _, f in plain])
        assert np.array_equal(np.stack([f for _, f in nv12]), want)
        vs.reset()
        assert lib.pfnl_stream_resize(vs._s, 0, 0) == 0                         # before a first frame: the network's size again, still NV12
        vs.out_size = None
        full = _stream_all(vs, lr)
        assert np.array_equal(np.stack([f for _, f in full]), np.stack([yuv.from_rgb(f, "nv12") for _, f in plain]))
        vs.reset()
        assert lib.pfnl_stream_format(vs._s, 0, 0, 1, 0) == 0                   # and the plain session's bytes
        vs.out_format = "rgb24"
        assert np.array_equal(np.stack([f for _, f in _stream_all(vs, lr)]), np.stack([f for _, f in plain]))
    for bad, fmt in [((15, 54), None), ((36, 193), None), ((37, 54), "nv12"), ((36, 55), "i420"), (36, None)]:
        with pytest.raises(ValueError):
            eng.open_stream(H, W, batch, out_format=fmt, out_size=bad)
    with eng.open_stream(H, W, batch, out_size=(37, 55)) as vs:                 # (nothing was left open by the refusals; odd sizes are fine as RGB)
        odd = _stream_all(vs, lr)
    assert np.array_equal(np.stack([f for _, f in odd]), np.stack([resize.resize(f, 37, 55) for _, f in plain]))
    eng.close()
