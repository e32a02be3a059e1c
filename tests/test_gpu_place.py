"""Placement on a canvas on a real MI355X (include/pfnl_hip.h PLACEMENT, pfnl_stream_place; pfnl_amd/csrc/place.hip): the kernels and the
session against the host rule pfnl_amd/fit.py place and pfnl_amd/depth10.py place10, byte for byte - no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfnl_amd import _capi, depth10, fit, ops, resize, surface, synth, yuv  # noqa: E402
from pfnl_amd.engine import PFNLEngine  # noqa: E402
from pfnl_amd.spec import PFNLGeometry  # noqa: E402

FILL = (16, 128, 235)
WHOLE = None
# frame, canvas, src, dst
CASES = {
    "words_edges_in_words": ((40, 72), (48, 144), WHOLE, (4, 19, 40, 101)),   # 16-byte stores, both edges of dst inside words; identity down,
                                                                              # 72 -> 101 across; three tile rows
    "crop_and_shrink": ((64, 96), (36, 64), (8, 12, 48, 72), (2, 8, 32, 48)),  # clamping at the crop's edges
    "odd_canvas": ((64, 96), (37, 55), WHOLE, (0, 3, 37, 49)),                 # the byte form; dst touches top and bottom
    "padding_only": ((64, 96), (80, 128), WHOLE, (8, 16, 64, 96)),             # dst.y no multiple of 16
    "crop_only": ((64, 96), (32, 48), (16, 24, 32, 48), WHOLE),
    "one_row": ((64, 96), (48, 96), (10, 0, 3, 96), (20, 0, 1, 96)),
    "quarter_and_bar_tiles": ((64, 96), (64, 160), WHOLE, (24, 8, 16, 24)),    # 4 : 1, 16 taps; tiles wholly in the bars
}


def _dev(a):
    """a numpy array on the device; uint16 through int16 (the copy kernels all know that type)"""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16) if a.dtype == np.uint16 else torch.from_numpy(a).cuda()


def _host(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16) if t.dtype == torch.uint16 else t.cpu().numpy()


def _samples_with_all_values(rng, shape, levels):
    a = rng.integers(0, levels, size=shape).astype(np.uint8 if levels == 256 else np.uint16)
    flat = a.reshape(-1)
    if flat.size >= levels:
        flat[rng.permutation(flat.size)[:levels]] = np.arange(levels, dtype=a.dtype)
    return a


def _frames(n, H, W, depth, seed):
    """n frames of random samples with every value present (where the frame has room); the last one blocks of 2 x 2 at the two extremes"""
    levels = 1 << depth
    rng = np.random.default_rng(seed)
    frames = [_samples_with_all_values(rng, (H, W, 3), levels) for _ in range(n)]
    small = rng.integers(0, 2, size=((H + 1) // 2, (W + 1) // 2, 3)).astype(frames[0].dtype) * (levels - 1)
    frames[-1] = np.repeat(np.repeat(small, 2, axis=0), 2, axis=1)[:H, :W]
    return np.stack(frames)


def _depth(depth):
    """(the op, the host rule on one frame with an 8-bit fill, the fill in the op's sample values)"""
    if depth == 8:
        return ops.resize_place_u8, fit.place, lambda f: tuple(f)
    return ops.resize_place_u10, depth10.place10, depth10.fill10


# ---- 1. the op --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("case", sorted(CASES))
def test_place_equals_the_host_rule(case, depth):
    (H, W), (oH, oW), src, dst = CASES[case]
    op, rule, samples = _depth(depth)
    sy, sx, sh, sw = src or (0, 0, H, W)
    for n in (1, 3):
        frames = _frames(n, H, W, depth, seed=H * 1000 + W + n)
        dev = _dev(frames)
        for fill in (FILL, (0, 0, 0)):
            want = np.stack([rule(f, oH, oW, src, dst, fill) for f in frames])
            got = _host(op(dev, (oH, oW), src, dst, samples(fill)))
            assert got.dtype == frames.dtype and got.shape == want.shape == (n, oH, oW, 3)
            assert np.array_equal(got, want), (case, depth, n, fill, int((got != want).sum()))
        if src is not None:                                                     # the pixels outside src never reach the output
            other = _frames(n, H, W, depth, seed=99)
            other[:, sy:sy + sh, sx:sx + sw] = frames[:, sy:sy + sh, sx:sx + sw]
            assert not np.array_equal(other, frames)
            again = _host(op(_dev(other), (oH, oW), src, dst, samples((0, 0, 0))))
            assert np.array_equal(again, want), (case, depth, n)
    if dst is not None:                                                         # (the cases have bars, and the bars are the fill)
        dy, dx, dh, dw = dst
        bars = np.ones((oH, oW), bool)
        bars[dy:dy + dh, dx:dx + dw] = False
        assert bars.any() and (got[:, bars] == 0).all()
    single = op(dev[0], (oH, oW), src, dst)                                     # [H,W,3] is a batch of one; the default fill is black
    assert tuple(single.shape) == (1, oH, oW, 3) and np.array_equal(_host(single)[0], want[0])


@pytest.mark.parametrize("depth", [8, 10])
def test_whole_rectangles_are_the_resize(depth):
    frames = _frames(2, 64, 96, depth, seed=3)
    dev = _dev(frames)
    op, plain, rule = (ops.resize_place_u8, ops.resize_u8, resize.resize) if depth == 8 else (ops.resize_place_u10, ops.resize_u10, depth10.resize10)
    for size in [(36, 54), (128, 192), (64, 96)]:
        want = _host(plain(dev, size))
        assert np.array_equal(want, np.stack([rule(f, *size) for f in frames]))   # both hooks launch one kernel: the host rule is the reference
        assert np.array_equal(_host(op(dev, size)), want)
        assert np.array_equal(_host(op(dev, size, (0, 0, 64, 96), (0, 0, *size), (1, 2, 3))), want)


@pytest.mark.parametrize("depth", [8, 10])
def test_unaligned_pointers_take_the_sample_form_and_stay_inside_the_destination(depth):
    """the case whose aligned form stores 16-byte words, with `in` and `out` moved off their alignment and guard samples around `out`"""
    (H, W), (oH, oW), src, dst = CASES["words_edges_in_words"]
    op, rule, samples = _depth(depth)
    n, slack = 2, 64
    dtype = np.uint8 if depth == 8 else np.uint16
    ob = n * oH * oW * 3
    frames = _frames(n, H, W, depth, seed=7)
    want = np.stack([rule(f, oH, oW, src, dst, FILL) for f in frames])
    for off in (0, 1, 4):                                                       # in samples (0 keeps slack + ob: the words end where the frames end)
        s = _dev(np.concatenate([np.zeros(off, dtype), frames.reshape(-1)]))
        guard = ((np.arange(slack + off + ob + slack) * 7 + 3) % (1 << depth)).astype(dtype)
        d = _dev(guard)
        lo = slack + off
        assert (s.data_ptr() + off * s.element_size()) % 16 == (off * s.element_size()) % 16 == (d.data_ptr() + lo * d.element_size()) % 16
        op(s[off:].view(n, H, W, 3), (oH, oW), src, dst, samples(FILL), out=d[lo:lo + ob])
        got = _host(d)
        assert np.array_equal(got[lo:lo + ob].reshape(want.shape), want), (depth, off)
        assert np.array_equal(got[:lo], guard[:lo]) and np.array_equal(got[lo + ob:], guard[lo + ob:]), (depth, off)


def test_wrong_arguments_raise():
    x = torch.zeros((2, 16, 24, 3), dtype=torch.uint8, device="cuda")
    x10 = torch.zeros((2, 16, 24, 3), dtype=torch.uint16, device="cuda")
    for op, t, other in ((ops.resize_place_u8, x, x10), (ops.resize_place_u10, x10, x)):
        with pytest.raises(ValueError):
            op(t, (32, 48), None, (4, 4, 16, 24), out=torch.zeros(2 * 32 * 48 * 3 + 1, dtype=t.dtype, device="cuda"))
        for bad in [dict(src=(0, 0, 17, 24)), dict(dst=(0, 30, 16, 24)), dict(dst=(0, 0, 3, 24)), dict(dst=(0, 0, 33, 48)), dict(fill=(0, 0, -1)),
                    dict(fill=(0, 0, 256 if t is x else 1024)), dict(src=(0, 0, 16)), dict(fill=(1, 2))]:
            with pytest.raises(ValueError):
                op(t, (32, 48), **bad)
        with pytest.raises(ValueError):
            op(torch.zeros((2, 16, 24, 2), dtype=t.dtype, device="cuda"), (32, 48))
        with pytest.raises(ValueError):
            op(t, (0, 48))
        with pytest.raises(TypeError):
            op(torch.zeros((2, 16, 24, 3), dtype=t.dtype), (32, 48))
        with pytest.raises(TypeError):
            op(other, (32, 48))
        with pytest.raises((TypeError, ValueError)):
            op(t, (32, 48), out=torch.zeros((2, 32, 48, 3), dtype=t.dtype))


# ---- 2. the session ---------------------------------------------------------------------------------------------------------------------
H, W = 16, 24                                                                   # the network delivers 64 x 96


@pytest.fixture(scope="module")
def engines():
    geom = PFNLGeometry(num_block=1)
    w = synth.synthetic_weights(geom, seed=0)
    pair = []
    for _ in range(2):
        e = PFNLEngine(geom, device=0)
        e.load_weights(w)
        pair.append(e)
    yield pair
    for e in pair:
        e.close()


def _lr(F, seed):
    return list(np.random.default_rng(seed).integers(0, 256, (F, H, W, 3), np.uint8))


def _stream_all(vs, frames, device=False):
    """push one frame at a time, pop after every push, then end: the delivered frames in order, as numpy"""
    got = []
    for f in frames:
        got += vs.push(torch.from_numpy(f).cuda() if device else f)
        got += vs.pop_ready()
    got += vs.end()
    assert [i for i, _ in got] == list(range(len(frames)))
    if device:
        assert all(torch.is_tensor(f) and f.is_cuda for _, f in got)
        return np.stack([_host(f) for _, f in got])
    return np.stack([f for _, f in got])


def _plain(engine, frames, batch, **kw):
    with engine.open_stream(H, W, batch, **kw) as vs:
        assert vs.crop is None and vs.place is None and vs.fill == (0, 0, 0)
        return _stream_all(vs, frames)


def test_pillarbox(engines):
    eng, eng2 = engines
    lr = _lr(6, 11)
    plain = _plain(eng2, lr, 2)
    assert plain.shape == (6, 64, 96, 3) and len(np.unique(plain)) > 16          # (frames with content)
    for fill in ((0, 0, 0), FILL):
        with eng.open_stream(H, W, 2, out_size=(64, 160), fit="contain", fill=fill) as vs:
            assert (vs.out_size, vs.crop, vs.place, vs.fill) == ((64, 160), (0, 0, 64, 96), (0, 32, 64, 96), fill)
            got = _stream_all(vs, lr)
        assert got.dtype == np.uint8 and got.shape == (6, 64, 160, 3)
        assert np.array_equal(got, np.stack([fit.place(f, 64, 160, None, (0, 32, 64, 96), fill) for f in plain]))
        assert np.array_equal(got[:, :, 32:128], plain)                         # the picture bytes are the plain session's own,
        assert (got[:, :, :32] == np.array(fill, np.uint8)).all() and (got[:, :, 128:] == np.array(fill, np.uint8)).all()   # the bars the fill


def test_crop_to_nv12(engines):
    eng, eng2 = engines
    lr = _lr(5, 12)
    plain = _plain(eng2, lr, 3)
    want = np.stack([yuv.from_rgb(fit.place(f, 36, 96, (8, 0, 48, 96), None), "nv12", "bt601") for f in plain])
    with eng.open_stream(H, W, 3, out_format="nv12", matrix="bt601", out_size=(36, 96), crop=(8, 0, 48, 96)) as vs:
        assert (vs.out_size, vs.crop, vs.place) == ((36, 96), (8, 0, 48, 96), (0, 0, 36, 96))
        got = _stream_all(vs, lr)
    assert got.shape == want.shape == (5, 54, 96) and np.array_equal(got, want)
    with eng.open_stream(H, W, 3, crop=(8, 0, 48, 96)) as vs:                   # a crop without a size: the crop at its own size
        assert vs.out_size == (48, 96)
        assert np.array_equal(_stream_all(vs, lr), plain[:, 8:56])


@pytest.mark.parametrize("F,batch", [(9, 4), (2, 5)])
def test_explicit_placement_to_p010(engines, F, batch):
    eng, eng2 = engines
    lr = _lr(F, 13)
    sr = _plain(eng2, lr, batch, out_format="rgb10")                            # quantise10 of the network's result, as the session makes it
    assert sr.dtype == np.uint16 and sr.shape == (F, 64, 96, 3)
    want = np.stack([depth10.from_rgb10(depth10.place10(f, 48, 128, None, (6, 16, 36, 54), FILL), "p010", "bt709") for f in sr])
    with eng.open_stream(H, W, batch, out_format="p010", out_size=(48, 128), place=(6, 16, 36, 54), fill=FILL) as vs:
        assert (vs.out_size, vs.crop, vs.place, vs.fill) == ((48, 128), (0, 0, 64, 96), (6, 16, 36, 54), FILL)
        for device in (False, True):
            got = _stream_all(vs, lr, device)
            assert got.dtype == np.uint16 and got.shape == want.shape == (F, 72, 128)
            assert np.array_equal(got, want), (device, int((got != want).sum()))
            vs.reset()                                                          # the setting survives
        # one frame through pop_planes into a pitched surface: the samples, and nothing between a row's end and the pitch
        shapes = surface.plane_shapes("p010", 48, 128)
        rows = [n * dt.itemsize for _, n, dt in shapes]
        pats = [((np.arange(nrows * (r + 64)) * 5 + 1) % 256).astype(np.uint8).reshape(nrows, r + 64) for (nrows, _, _), r in zip(shapes, rows)]
        bufs = [torch.from_numpy(p).cuda() for p in pats]
        views = surface.views(bufs, "p010", 48, 128)
        delivered = sum(len(vs.push(torch.from_numpy(f).cuda())) for f in lr)       # (push hands over the batches launched before it)
        _capi.check(vs._lib.pfnl_stream_end(vs._handle()))
        assert vs.pop_planes(*views) == delivered < F
        torch.cuda.current_stream().synchronize()
        now = [b.cpu().numpy() for b in bufs]
        assert all(np.array_equal(g, w_) for g, w_ in zip(surface.extract(now, "p010", 48, 128), surface.split(want[delivered], "p010", 48, 128)))
        assert all(np.array_equal(b[:, r:], p[:, r:]) for b, p, r in zip(now, pats, rows))


def test_refusals_and_replacement(engines):
    eng, eng2 = engines
    lib, R = eng._lib, _capi.rect_arg
    lr = _lr(6, 14)
    plain = _plain(eng2, lr, 2)
    placed = np.stack([fit.place(f, 48, 128, None, (6, 16, 36, 54), FILL) for f in plain])
    fill = (C.c_uint8 * 3)(*FILL)
    with eng.open_stream(H, W, 2, out_size=(48, 128), place=(6, 16, 36, 54), fill=FILL) as vs:
        s = vs._s
        got = list(vs.push(lr[0]))
        assert lib.pfnl_stream_place(s, 0, 0, None, None, None) == -2 and b"before the first frame" in lib.pfnl_last_error()   # PFNL_ERR_STATE
        assert lib.pfnl_stream_place(s, 64, 160, None, R((0, 32, 64, 96)), fill) == -2
        assert lib.pfnl_stream_resize(s, 36, 54) == -2
        assert lib.pfnl_stream_place(s, 64, 160, None, R((0, 100, 64, 96)), fill) == -1 and b"dst" in lib.pfnl_last_error()    # PFNL_ERR_INVALID,
        assert lib.pfnl_stream_place(s, 64, 160, R((0, 0, 65, 96)), None, fill) == -1 and b"src" in lib.pfnl_last_error()      # at any time
        assert lib.pfnl_stream_place(s, 0, 0, None, R((0, 0, 8, 8)), None) == -1 and b"canvas" in lib.pfnl_last_error()
        got += vs.pop_ready()                                                   # ... and nothing changed: the sequence carries on
        for f in lr[1:]:
            got += vs.push(f)
            got += vs.pop_ready()
        got += vs.end()
        assert [i for i, _ in got] == list(range(6)) and np.array_equal(np.stack([f for _, f in got]), placed)
        vs.reset()
        # refusals before a first frame change nothing either
        assert lib.pfnl_stream_place(s, 48, 128, None, R((0, 0, 8, 54)), fill) == -1 and b"quarter" in lib.pfnl_last_error()
        assert lib.pfnl_stream_place(s, 20000, 128, None, R((6, 16, 36, 54)), fill) == -1
        assert np.array_equal(_stream_all(vs, lr), placed)
        vs.reset()
        # a 4:2:0 format needs an even canvas, whichever call comes second; the rectangles need not be even
        assert lib.pfnl_stream_place(s, 47, 128, None, R((6, 16, 36, 54)), fill) == 0
        assert lib.pfnl_stream_format(s, 0, 1, 1, 0) == -1 and b"even" in lib.pfnl_last_error()
        assert lib.pfnl_stream_place(s, 48, 128, None, R((5, 17, 37, 53)), fill) == 0 and lib.pfnl_stream_format(s, 0, 1, 1, 0) == 0
        assert lib.pfnl_stream_place(s, 47, 128, None, R((6, 16, 36, 54)), fill) == -1 and b"even" in lib.pfnl_last_error()
        vs.out_format = "nv12"                                                  # (the raw calls went past the Python object)
        want = np.stack([yuv.from_rgb(fit.place(f, 48, 128, None, (5, 17, 37, 53), FILL), "nv12", "bt709") for f in plain])
        assert np.array_equal(_stream_all(vs, lr), want)
        vs.reset()
        assert lib.pfnl_stream_format(s, 0, 0, 1, 0) == 0
        vs.out_format = "rgb24"
        # pfnl_stream_resize replaces a placement: the plain stretch
        assert lib.pfnl_stream_resize(s, 36, 54) == 0
        vs.out_size = (36, 54)
        stretch = _stream_all(vs, lr)
        vs.reset()
        # all-NULL rectangles, and rectangles that cover raster and canvas, are that resize
        for src, dst in ((None, None), (R((0, 0, 64, 96)), R((0, 0, 36, 54)))):
            assert lib.pfnl_stream_place(s, 48, 128, None, R((6, 16, 36, 54)), fill) == 0      # (a placement in between)
            assert lib.pfnl_stream_place(s, 36, 54, src, dst, fill) == 0
            assert np.array_equal(_stream_all(vs, lr), stretch)
            vs.reset()
        # and a placement replaces a resize; (0, 0, NULL, NULL, NULL) is off
        assert lib.pfnl_stream_place(s, 48, 128, None, R((6, 16, 36, 54)), fill) == 0
        vs.out_size = (48, 128)
        assert np.array_equal(_stream_all(vs, lr), placed)
        vs.reset()
        assert lib.pfnl_stream_place(s, 0, 0, None, None, None) == 0
        vs.out_size = None
        assert np.array_equal(_stream_all(vs, lr), plain)
    with eng2.open_stream(H, W, 2, out_size=(36, 54)) as vs:                    # the stretch is the resized session's
        assert np.array_equal(_stream_all(vs, lr), stretch)
    for bad in [dict(out_size=(64, 160), fit="contain", place=(0, 32, 64, 96)), dict(out_size=(64, 160), place=(0, 100, 64, 96)),
                dict(out_size=(37, 54), out_format="nv12", fit="contain"), dict(out_size=(64, 160), place=(0, 0, 8, 8)), dict(crop=(0, 0, 65, 96))]:
        with pytest.raises(ValueError):
            eng.open_stream(H, W, 2, **bad)
    with eng.open_stream(H, W, 2) as vs:                                        # (nothing was left open by the refusals)
        assert np.array_equal(_stream_all(vs, lr), plain)


def test_recomputed_batches_leave_placed():
    """The range fence (tests/test_gpu_resize.py test_recomputed_batches_leave_resized: conv0 x 4e5 leaves binary16's range, convmerge2 x 1e-6
    brings the result back to bytes): the batches the session computes again on the strict kernels are placed - and converted - like any other."""
    h, w, batch = 12, 20, 3                                                     # the network delivers 48 x 80
    lr = list(np.random.default_rng(21).integers(0, 256, size=(7, h, w, 3), dtype=np.uint8))
    geom = PFNLGeometry(num_block=1)
    weights = synth.synthetic_weights(geom, seed=1)
    weights["nlvsr/conv0/kernel"] = (weights["nlvsr/conv0/kernel"] * 4e5).astype(np.float32)
    weights["nlvsr/convmerge2/kernel"] = (weights["nlvsr/convmerge2/kernel"] * 1e-6).astype(np.float32)
    pair = []
    for _ in range(2):
        e = PFNLEngine(geom, device=0)
        e.load_weights(weights)
        pair.append(e)
    eng, eng2 = pair
    with eng2.open_stream(h, w, batch) as vs:
        plain = _stream_all(vs, lr)
    assert eng2.range_flagged() is False
    want = np.stack([fit.place(f, 40, 80, (2, 4, 44, 72), (4, 10, 30, 54), FILL) for f in plain])
    assert len(np.unique(want[:, 4:34, 10:64])) > 16                            # (frames with content, not a flat failure value)
    for fmt in ("rgb24", "nv12"):
        with eng.open_stream(h, w, batch, out_format=fmt, out_size=(40, 80), crop=(2, 4, 44, 72), place=(4, 10, 30, 54), fill=FILL) as vs:
            got = _stream_all(vs, lr)
            assert eng.get_option("strict_fp32") == "off"                       # end + the last pop have put it back
        expect = want if fmt == "rgb24" else np.stack([yuv.from_rgb(f, fmt) for f in want])
        assert np.array_equal(got, expect), fmt
    for e in pair:
        e.close()
