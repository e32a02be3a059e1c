"""Surfaces on a real MI355X (include/pfnl_hip.h SURFACES; pfnl_amd/surface.py): planes by pointer and row pitch into the decode kernel,
into the session (push_planes) and out of it (pop_planes), host and device.  Every comparison is byte for byte - against pfnl_amd/yuv.py for
the kernel, against the packed session for the session - and every byte between a row's end and its pitch is accounted for."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import streams as St  # noqa: E402
import test_gpu_scene as TSC  # noqa: E402   (content with cuts)
import test_gpu_yuv as TY  # noqa: E402   (packed 4:2:0 frames with every byte value and the extremes; the shapes)
from pfnl_amd import _capi, ops, surface, synth, yuv  # noqa: E402
from pfnl_amd.engine import PFNLEngine  # noqa: E402
from pfnl_amd.spec import PFNLGeometry  # noqa: E402

H, W, BATCH = 16, 24, 2                                  # the session geometry of the stream tests: sH x sW = 64 x 96
PUSH_D_MS = 5.0


def _up64(n):
    return (n + 63) // 64 * 64


def _pattern(shape):
    return ((np.arange(int(np.prod(shape)), dtype=np.int64) * 7 + 3) & 255).astype(np.uint8).reshape(shape)


# pitch of plane k for a row of r bytes: packed, odd, 4-byte words at most, a decoder's rounding, and another one for every plane
PITCHES = {"packed": lambda r, k: r, "plus1": lambda r, k: r + 1, "plus4": lambda r, k: r + 4, "up64": lambda r, k: _up64(r) + 64,
           "per_plane": lambda r, k: (_up64(r) + 64, r + 2, r + 16)[k]}


def _pitches(fmt, h, w, rule):
    return [rule(n * dt.itemsize, k) for k, (_, n, dt) in enumerate(surface.plane_shapes(fmt, h, w))]


def _device_surface(planes, pitches, fill, fmt, h, w):
    """the planes in pitched buffers of their own on the device -> (buffers, strided plane views)"""
    bufs = [torch.from_numpy(b).cuda() for b in surface.embed(planes, pitches, fill)]
    return bufs, surface.views(bufs, fmt, h, w)


@pytest.fixture(scope="module")
def eng():
    geom = PFNLGeometry(num_block=1)
    e = PFNLEngine(geom, device=0)
    e.load_weights(synth.synthetic_weights(geom, seed=0))
    yield e
    e.close()
    St.teardown()


# ---- 1. the op against the rule ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", yuv.FORMATS)
@pytest.mark.parametrize("h,w", TY.SHAPES)
def test_surface_op_equals_the_host_rule_at_any_pitch(h, w, fmt):
    for frame in TY._yuv_frames(2, h, w, fmt, seed=h * 1000 + w):                          # random bytes with every value; the extreme planes
        _check_surface_op(frame, h, w, fmt)


def _check_surface_op(frame, h, w, fmt):
    planes = surface.split(frame, fmt, h, w)
    want = {p: yuv.to_rgb(frame, fmt, h, w, *p) for p in TY.PAIRS}
    off, rb, slack = 16, h * w * 3, 64
    pat = _pattern((off + rb + slack,))
    packed = ops.yuv420_to_rgb(torch.from_numpy(frame).cuda(), fmt, h, w, "bt601", False).cpu().numpy()[0]
    assert np.array_equal(packed, want[("bt601", False)])
    for name, rule in PITCHES.items():
        pitches = _pitches(fmt, h, w, rule)
        per_fill = []
        for fill in (0x00, 0xFF):
            _, vs = _device_surface(planes, pitches, fill, fmt, h, w)
            assert surface.describe(vs, fmt, h, w)[1] == pitches
            outs = {}
            for matrix, full in TY.PAIRS:
                dst = torch.from_numpy(pat).cuda()
                got = ops.yuv420_to_rgb_surface(vs, fmt, h, w, matrix, full, out=dst[off:off + rb])
                assert got.shape == (h, w, 3) and got.dtype == torch.uint8
                whole = dst.cpu().numpy()
                outs[(matrix, full)] = whole[off:off + rb].reshape(h, w, 3)
                assert np.array_equal(outs[(matrix, full)], want[(matrix, full)]), (h, w, fmt, name, matrix, full,
                                                                                     int((outs[(matrix, full)] != want[(matrix, full)]).sum()))
                assert np.array_equal(whole[:off], pat[:off]) and np.array_equal(whole[off + rb:], pat[off + rb:]), (name, "outside [H][W][3]")
            per_fill.append(outs)
        assert all(np.array_equal(per_fill[0][p], per_fill[1][p]) for p in TY.PAIRS), (name, "the padding's bytes reached the result")
        if name == "packed":
            assert np.array_equal(per_fill[0][("bt601", False)], packed)                 # pitch = W is the packed op
    got = ops.yuv420_to_rgb_surface(_device_surface(planes, _pitches(fmt, h, w, PITCHES["up64"]), 0x5A, fmt, h, w)[1], fmt, h, w, "bt709", True)
    assert np.array_equal(got.cpu().numpy(), want[("bt709", True)])                      # and it allocates its own result


# ---- 2. a window of a larger surface -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", yuv.FORMATS)
@pytest.mark.parametrize("y0,x0", [(2, 2), (4, 6), (4, 16)])   # plane pointers at 2 mod 4, at 2 mod 4 with another chroma offset, at 0 mod 16
def test_a_window_of_a_surface_is_the_cropped_frame(y0, x0, fmt):
    SHs, SWs, h, w = 24, 64, 10, 36
    rng = np.random.default_rng(100 * y0 + x0)
    Y, Cb, Cr = TY._bytes_with_all_values(rng, (SHs, SWs)), TY._bytes_with_all_values(rng, (SHs // 2, SWs // 2)), TY._bytes_with_all_values(rng, (SHs // 2, SWs // 2))
    crop = yuv.pack(Y[y0:y0 + h, x0:x0 + w], Cb[y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2], Cr[y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2], fmt)
    dY = torch.from_numpy(Y).cuda()
    if fmt == "nv12":
        dC = torch.from_numpy(np.stack([Cb, Cr], axis=2).reshape(SHs // 2, SWs)).cuda()
        vs = (dY[y0:y0 + h, x0:x0 + w], dC[y0 // 2:(y0 + h) // 2, x0:x0 + w])
        assert surface.describe(vs, fmt, h, w)[1] == [SWs, SWs]
    else:
        dB, dR = torch.from_numpy(Cb).cuda(), torch.from_numpy(Cr).cuda()
        vs = (dY[y0:y0 + h, x0:x0 + w], dB[y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2], dR[y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2])
        assert surface.describe(vs, fmt, h, w)[1] == [SWs, SWs // 2, SWs // 2]
    assert surface.describe(vs, fmt, h, w)[0][0] == dY.data_ptr() + y0 * SWs + x0
    for matrix, full in TY.PAIRS:
        got = ops.yuv420_to_rgb_surface(vs, fmt, h, w, matrix, full).cpu().numpy()
        want = yuv.to_rgb(crop, fmt, h, w, matrix, full)                                 # chroma clamps at the window's edges, not the surface's
        assert np.array_equal(got, want), (fmt, y0, x0, matrix, full, int((got != want).sum()))


# ---- the sessions' helpers -----------------------------------------------------------------------------------------------------------------
def _run(vs, pushes):
    """pushes: one callable per frame.  Pops one frame at a time after every push: ([index], [frame as numpy], [last_info], cuts)"""
    idx, frames, infos = [], [], []

    def drain():
        while vs.ready():
            i, f = vs.pop()
            idx.append(i), frames.append(St.to_numpy(St._as_int(f).cpu(), f) if torch.is_tensor(f) else f), infos.append(vs.last_info)

    for push in pushes:
        assert push() == []                                                              # (everything deliverable was popped before)
        drain()
    _capi.check(vs._lib.pfnl_stream_end(vs._handle()))
    drain()
    return idx, frames, infos, list(vs.cuts)


def _input_frames(fmt, F=7):
    """a sequence with one cut, packed in `fmt`"""
    rgb = TSC._scenes_u8((4, F - 4), seed=61, h=H, w=W)
    return list(rgb) if fmt == "rgb24" else [yuv.from_rgb(f, fmt, "bt601", False) for f in rgb]


def _planes_push(vs, frame, fmt, device, rule, fill=0xA5):
    """push_planes of a packed frame's planes, each embedded in a pitched buffer of its own (chroma allocated apart from luma)"""
    planes = surface.split(frame, fmt, H, W)
    pitches = _pitches(fmt, H, W, rule)
    if device:
        _, views = _device_surface(planes, pitches, fill, fmt, H, W)
    else:
        views = surface.views(surface.embed(planes, pitches, fill), fmt, H, W)
    return vs.push_planes(*views)


# ---- 3. the session, input side -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["rgb24", "nv12", "i420"])
def test_push_planes_delivers_the_packed_sessions_frames(eng, fmt):
    frames = _input_frames(fmt)
    kw = dict(pixel_format=fmt, out_format="rgb24", matrix="bt601", scene_cut=10.0)
    with eng.open_stream(H, W, BATCH, **kw) as vs:
        ref = _run(vs, [lambda f=f: vs.push(f) for f in frames])
        assert ref[0] == list(range(len(frames))) and ref[3] == [4]                      # the cut is seen
        for device in (False, True):
            for name in ("up64", "per_plane", "plus1"):
                vs.reset()
                got = _run(vs, [lambda f=f: _planes_push(vs, f, fmt, device, PITCHES[name]) for f in frames])
                assert got[0] == ref[0] and got[2] == ref[2] and got[3] == ref[3], (fmt, device, name, got[2], ref[2])
                assert np.array_equal(np.stack(got[1]), np.stack(ref[1])), (fmt, device, name)
        vs.reset()                                                                       # push and push_planes alternate; host and device alternate
        mixed = [(lambda f=f: vs.push(f)) if k % 2 else (lambda f=f, k=k: _planes_push(vs, f, fmt, k % 4 == 0, PITCHES["up64"]))
                 for k, f in enumerate(frames)]
        got = _run(vs, mixed)
        assert got[0] == ref[0] and got[2] == ref[2] and got[3] == ref[3]
        assert np.array_equal(np.stack(got[1]), np.stack(ref[1]))


# ---- 4. the session, output side -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_size", [None, (40, 72)])
@pytest.mark.parametrize("out_fmt", ["rgb24", "nv12", "i420", "rgb10", "p010", "i010"])
def test_pop_planes_writes_the_packed_sessions_samples_and_nothing_else(eng, out_fmt, out_size):
    frames = list(np.random.default_rng(71).integers(0, 256, (5, H, W, 3), np.uint8))
    oH, oW = out_size or (4 * H, 4 * W)
    shapes = surface.plane_shapes(out_fmt, oH, oW)
    rows = [n * dt.itemsize for _, n, dt in shapes]
    pitches = [(_up64(r) + 64, r + 2, r + 10)[k] for k, r in enumerate(rows)]            # (even: 16-bit samples need that)
    pats = [_pattern((nrows, p)) for (nrows, _, _), p in zip(shapes, pitches)]
    with eng.open_stream(H, W, BATCH, out_format=out_fmt, out_size=out_size) as vs:
        ref = _run(vs, [lambda f=f: vs.push(f) for f in frames])
        assert ref[0] == list(range(5)) and ref[1][0].dtype == (np.uint16 if out_fmt in _capi.TEN_BIT_FORMATS else np.uint8)
        for device in (False, True):
            vs.reset()
            bufs = [torch.from_numpy(p).cuda() for p in pats] if device else [p.copy() for p in pats]
            host = (lambda: [b.cpu().numpy() for b in bufs]) if device else (lambda: bufs)
            views = surface.views(bufs, out_fmt, oH, oW)
            assert surface.describe(views, out_fmt, oH, oW)[1] == pitches
            assert vs.pop_planes(*views) is None                                         # nothing deliverable: nothing written
            assert all(np.array_equal(b, p) for b, p in zip(host(), pats))
            idx = []
            for k, f in enumerate(frames + [None]):
                if f is None:
                    _capi.check(vs._lib.pfnl_stream_end(vs._handle()))
                else:
                    assert (vs.push(torch.from_numpy(f).cuda()) if device else vs.push(f)) == []
                while vs.ready():
                    for b, p in zip(bufs, pats):                                         # a fresh pattern under every frame
                        b.copy_(torch.from_numpy(p)) if device else np.copyto(b, p)
                    i = vs.pop_planes(*views)
                    if device:
                        torch.cuda.current_stream().synchronize()
                    idx.append(i)
                    now = host()
                    want = surface.split(ref[1][i], out_fmt, oH, oW)
                    got = surface.extract(now, out_fmt, oH, oW)
                    assert all(g.dtype == w_.dtype and np.array_equal(g, w_) for g, w_ in zip(got, want)), (out_fmt, out_size, device, i)
                    assert all(np.array_equal(b[:, r:], p[:, r:]) for b, p, r in zip(now, pats, rows)), (out_fmt, out_size, device, i, "padding")
                    assert vs.last_info == (0, 0)
            assert idx == list(range(5))
            assert vs.pop_planes(*views) is None


# ---- 5. errors change nothing --------------------------------------------------------------------------------------------------------------
def test_refused_surfaces_change_nothing_and_the_bound_holds(eng):
    fmt, frames = "nv12", _input_frames("nv12", F=6)
    lib = eng._lib
    with eng.open_stream(H, W, BATCH, pixel_format=fmt, matrix="bt601") as vs:
        ref = _run(vs, [lambda f=f: vs.push(f) for f in frames])
        vs.reset()
        oH, oW = 4 * H, 4 * W
        out_bufs = [np.zeros((oH, oW + 64), np.uint8), np.zeros((oH // 2, oW + 64), np.uint8)]
        out_views = surface.views(out_bufs, fmt, oH, oW)

        def refusals():
            planes = surface.split(frames[0], fmt, H, W)
            good = surface.as_struct(planes, fmt, H, W)
            short = _capi.pfnl_surface(good.plane, (C.c_size_t * 3)(W, W - 1, 0))
            assert lib.pfnl_stream_push_surface(vs._s, C.byref(short), 0) == -1 and b"pitch" in lib.pfnl_last_error()
            holed = _capi.pfnl_surface((C.c_void_p * 3)(good.plane[0], None, None), good.pitch)
            assert lib.pfnl_stream_push_surface(vs._s, C.byref(holed), 0) == -1 and b"plane" in lib.pfnl_last_error()
            out = surface.as_struct(out_views, fmt, oH, oW)
            short = _capi.pfnl_surface(out.plane, (C.c_size_t * 3)(oW - 1, oW + 64, 0))
            index, got = C.c_longlong(-5), C.c_int(-5)
            assert lib.pfnl_stream_pop_surface(vs._s, C.byref(short), 0, C.byref(index), C.byref(got)) == -1 and b"pitch" in lib.pfnl_last_error()
            assert (index.value, got.value) == (-5, -5)
            with pytest.raises(ValueError):
                vs.push_planes(planes[0])                                                # a wrong plane count
            with pytest.raises(ValueError):
                vs.push_planes(planes[0], planes[1], planes[1])
            with pytest.raises(ValueError):
                vs.push_planes(planes[0], planes[1][:, :W - 2])
            with pytest.raises(ValueError):
                vs.push_planes(planes[0], torch.from_numpy(planes[1]).cuda())            # host and device planes in one frame
            with pytest.raises(ValueError):
                vs.pop_planes(out_views[0])
            with pytest.raises(ValueError):
                vs.pop_planes(out_views[0], out_views[1][:, :oW - 2])
            assert not out_bufs[0].any() and not out_bufs[1].any()

        refusals()                                                                       # before the first frame,
        pushes = [lambda f=f: _planes_push(vs, f, fmt, False, PITCHES["up64"]) for f in frames]
        pushes[3] = lambda: (refusals(), _planes_push(vs, frames[3], fmt, False, PITCHES["up64"]))[1]   # and in the middle of the sequence
        got = _run(vs, pushes)
        assert got[0] == ref[0] and np.array_equal(np.stack(got[1]), np.stack(ref[1]))
    with eng.open_stream(H, W, 1, pixel_format=fmt) as vs:                               # "pop first", as test_readiness_and_the_undelivered_bound
        T = eng.geom.num_frames
        sfs = [surface.as_struct(surface.split(f, fmt, H, W), fmt, H, W) for f in frames]
        raw = lambda k: lib.pfnl_stream_push_surface(vs._s, C.byref(sfs[k % len(sfs)]), 0)   # noqa: E731
        for k in range(T // 2):
            assert raw(k) == 0 and vs.ready() == 0
        assert raw(T // 2) == 0 and vs.ready() == 1
        assert raw(T // 2 + 1) == 0 and vs.ready() == 2                                  # 2 * batch undelivered frames
        assert raw(T // 2 + 2) == -2 and b"pop first" in lib.pfnl_last_error() and vs.ready() == 2
        assert vs.pop()[0] == 0
        assert raw(T // 2 + 2) == 0 and vs.ready() == 2                                  # the refused frame, now accepted
        _capi.check(lib.pfnl_stream_end(vs._s))
        assert raw(0) == -2 and b"pfnl_stream_end" in lib.pfnl_last_error()              # push after end


# ---- 6. the stream contract ---------------------------------------------------------------------------------------------------------------
def test_device_planes_are_ordered_on_the_sessions_stream(eng):
    """The session opened under a non-blocking side stream S (tests/streams.py, Probe L): every frame's planes arrive late on S - behind a
    spin, over a completed 0xA5 fill - so a push_planes that read them ahead of S converts the fill; every pop_planes is followed on S by
    the copy of its destination to pinned memory, which sees the pattern if the delivery ran elsewhere."""
    fmt, F = "nv12", 6
    frames = _input_frames(fmt, F)
    oH, oW = 4 * H, 4 * W
    with eng.open_stream(H, W, BATCH, pixel_format=fmt, matrix="bt601") as vs:            # the reference: the default stream, packed frames
        ref = _run(vs, [lambda f=f: vs.push(torch.from_numpy(f).cuda()) for f in frames])
    assert ref[0] == list(range(F))
    S = St.side_stream()
    St.require("L")
    assert St.control_late(S, D=PUSH_D_MS), "insensitive on this device at the per-push delay"
    in_pitches, out_pitches = _pitches(fmt, H, W, PITCHES["up64"]), _pitches(fmt, oH, oW, PITCHES["up64"])
    real = [surface.embed(surface.split(f, fmt, H, W), in_pitches, 0x11) for f in frames]
    pins = [[St.pinned_like(b) for b in bufs] for bufs in real]
    src = [[torch.full(b.shape, 0xA5, dtype=torch.uint8, device="cuda") for b in bufs] for bufs in real]
    pats = [_pattern((rows, p)) for (rows, _, _), p in zip(surface.plane_shapes(fmt, oH, oW), out_pitches)]
    dst = [torch.from_numpy(p).cuda() for p in pats]
    landed = [[torch.zeros(p.shape, dtype=torch.uint8).pin_memory() for p in pats] for _ in range(F)]
    dviews = surface.views(dst, fmt, oH, oW)
    torch.cuda.synchronize()
    idx = []
    with torch.cuda.stream(S):
        vs = eng.open_stream(H, W, BATCH, pixel_format=fmt, matrix="bt601")
    try:
        with torch.cuda.stream(S):
            for k in range(F + 1):
                if k < F:
                    St.sleep_ms(PUSH_D_MS)
                    for b, p in zip(src[k], pins[k]):
                        b.view(-1).copy_(p, non_blocking=True)
                    assert vs.push_planes(*surface.views(src[k], fmt, H, W)) == []
                else:
                    _capi.check(vs._lib.pfnl_stream_end(vs._handle()))
                while vs.ready():
                    i = vs.pop_planes(*dviews)
                    for h_, d in zip(landed[i], dst):
                        h_.copy_(d, non_blocking=True)
                    idx.append(i)
        S.synchronize()
    finally:
        vs.close()
    assert idx == ref[0]
    rows = [n for _, n, _ in surface.plane_shapes(fmt, oH, oW)]
    for i in range(F):
        got = surface.extract([h_.numpy() for h_ in landed[i]], fmt, oH, oW)
        want = surface.split(ref[1][i], fmt, oH, oW)
        assert all(np.array_equal(g, w_) for g, w_ in zip(got, want)), f"frame {i}: push_planes / pop_planes were not ordered on the session's stream"
        assert all(np.array_equal(h_.numpy()[:, r:], p[:, r:]) for h_, p, r in zip(landed[i], pats, rows))
