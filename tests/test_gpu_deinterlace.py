"""Interlaced input on a real MI355X (include/pfnl_hip.h INTERLACED; pfnl_amd/csrc/deinterlace.hip): the kernel at both depths in its
16-byte, 4-byte and single-sample forms against pfnl_amd/deinterlace.py interpolate, and the session with the setting on - every input
family, host and device pushes, both rates and both field orders - against a progressive RGB session pushed with
deinterlace.frames(decode_fields(...)).  Byte for byte, no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import deint_gen  # noqa: E402
from pfnl_amd import _capi, deinterlace, depth10, ops, surface, synth, yuv  # noqa: E402
from pfnl_amd import packed as P  # noqa: E402
from pfnl_amd.engine import PFNLEngine  # noqa: E402
from pfnl_amd.spec import PFNLGeometry  # noqa: E402

# (H, W): every row index clamps; two pairs; the single-sample form (15 bytes a row; 30 at 10 bits: 2-byte samples); three 16-byte words a
# row at 8 bits; 66 bytes a row - the single-sample form at 8 bits, 4-byte words at 10 (132 bytes); 96 bytes; and a height above the
# strip (ops.DEINTERLACE_STRIP_ROWS rows) at W = 16: a strip boundary inside the frame, the last strip one pair short
OP_SHAPES = [(2, 1), (4, 2), (6, 5), (8, 16), (12, 22), (10, 32), (ops.DEINTERLACE_STRIP_ROWS + 2, 16)]
WIDE_SHAPES = [(8, 16), (10, 32), (ops.DEINTERLACE_STRIP_ROWS + 2, 16)]
H, W, BATCH, F = 16, 24, 2, 5                                            # the sessions: one block, sH x sW = 64 x 96


def _cuda(a):
    a = np.ascontiguousarray(a)                                          # (torch copies int16, not uint16)
    return torch.from_numpy(a).cuda() if a.dtype == np.uint8 else torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)


def _numpy(t):
    return t.cpu().numpy() if t.dtype == torch.uint8 else t.view(torch.int16).cpu().numpy().view(np.uint16)


def _op(maxv):
    return ops.deinterlace if maxv == 255 else ops.deinterlace_u10


def _fields(h, w, maxv, n=3, seed=None):
    seq = deinterlace.sequence_fields(deint_gen.woven_rgb(n, h, w, maxv, deint_gen.SEED if seed is None else seed))
    return [np.ascontiguousarray(f) for f, _ in seq], [p for _, p in seq]


# ---- the op ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("maxv", [255, 1023])
@pytest.mark.parametrize("h,w", OP_SHAPES)
def test_the_kernel_equals_interpolate(h, w, maxv):
    fields, parity = _fields(h, w, maxv)
    if maxv == 1023:                                                     # samples above 1023 are taken as 1023
        fields[1] = fields[1].copy()
        fields[1].reshape(-1)[::3] = np.array([1024, 2000, 32768, 65535], np.uint16)[np.arange(fields[1].size)[::3] % 4]
    dev = [_cuda(f) for f in fields]
    for k in (2, 3):                                                     # both parities, every neighbour a field of its own
        want = deinterlace.interpolate(fields[k - 2], fields[k - 1], fields[k], fields[k + 1], fields[k + 2], parity[k], maxv)
        got = _numpy(_op(maxv)(dev[k - 2], dev[k - 1], dev[k], dev[k + 1], dev[k + 2], parity[k]))
        assert got.shape == (h, w, 3) and got.dtype == want.dtype
        assert np.array_equal(got, want), (h, w, maxv, k, int((got != want).sum()))


@pytest.mark.parametrize("maxv", [255, 1023])
@pytest.mark.parametrize("h,w", OP_SHAPES)
def test_aliased_fields_as_at_a_sequences_ends(h, w, maxv):
    fields, parity = _fields(h, w, maxv, n=2)
    dev = [_cuda(f) for f in fields]
    for k in (0, 3):                                                     # P2 = cur, P1 = N1 | N2 = cur, N1 = P1
        a, b, c, d = deinterlace.neighbours(k, 4)
        want = deinterlace.interpolate(fields[a], fields[b], fields[k], fields[c], fields[d], parity[k], maxv)
        got = _numpy(_op(maxv)(dev[a], dev[b], dev[k], dev[c], dev[d], parity[k]))
        assert np.array_equal(got, want), (h, w, maxv, k)
    one = deinterlace.interpolate(fields[0], fields[1], fields[0], fields[1], fields[0], 0, maxv)   # a one-frame sequence is its own weave
    woven = np.empty_like(one)
    woven[0::2], woven[1::2] = np.minimum(fields[0], maxv), np.minimum(fields[1], maxv)
    assert np.array_equal(one, woven)
    assert np.array_equal(_numpy(_op(maxv)(dev[0], dev[1], dev[0], dev[1], dev[0], 0)), woven)


def _at_offset(a, off, fill):
    """``a`` in a device buffer of ``fill`` bytes, ``off`` bytes behind a 256-byte boundary, 64 bytes of ``fill`` behind it: (buffer, view)"""
    nbytes = a.size * a.itemsize
    buf = torch.full((off + nbytes + 64,), fill, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    raw = buf[off:off + nbytes]
    raw.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8)).cuda())
    view = raw if a.dtype == np.uint8 else raw.view(torch.uint16)
    return buf, view.view(a.shape)


@pytest.mark.parametrize("maxv", [255, 1023])
@pytest.mark.parametrize("off", [0, 4])
@pytest.mark.parametrize("h,w", WIDE_SHAPES)
def test_offset_pointers_and_a_guarded_output(h, w, off, maxv):
    """off = 4: every pointer 4 bytes off a 16-byte boundary - the 4-byte form on rows that would allow 16-byte words.  The output is
    pre-filled, and the bytes before and behind it stay what they were."""
    fields, parity = _fields(h, w, maxv, seed=7)
    held = [_at_offset(f, off, 0x5A) for f in fields]
    for k in (2, 3):
        want = deinterlace.interpolate(fields[k - 2], fields[k - 1], fields[k], fields[k + 1], fields[k + 2], parity[k], maxv)
        buf, out = _at_offset(np.full_like(want, 0x3C3C if maxv == 1023 else 0x3C), off, 0xA5)
        assert out.data_ptr() % 16 == off
        got = _op(maxv)(*(held[q][1] for q in range(k - 2, k + 3)), parity[k], out=out)
        assert got.data_ptr() == out.data_ptr()
        assert np.array_equal(_numpy(got), want), (h, w, off, maxv, k)
        raw = buf.cpu().numpy()
        assert (raw[:off] == 0xA5).all() and (raw[off + want.size * want.itemsize:] == 0xA5).all()
    for (buf, view), f in zip(held, fields):                            # the fields are only read
        assert np.array_equal(_numpy(view), f)


def test_the_hooks_refuse_by_name():
    lib = _capi.load_library()
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    ok = [p, p + 256, p + 512, p + 768, p + 1024, 4, 2, 0, p + 2048, None]
    assert lib.pfnl_op_deinterlace_u8(*ok) == 0
    for at, name in enumerate((b"p2", b"p1", b"cur", b"n1", b"n2")):
        bad = list(ok)
        bad[at] = None
        assert lib.pfnl_op_deinterlace_u8(*bad) == -1 and name in lib.pfnl_last_error()
    for at, value, name in ((5, 3, b"H"), (5, 0, b"H"), (6, 0, b"W"), (7, 2, b"parity"), (8, None, b"out")):
        bad = list(ok)
        bad[at] = value
        assert lib.pfnl_op_deinterlace_u10(*bad) == -1 and name in lib.pfnl_last_error()
    bad = list(ok)
    bad[2] = p + 513
    assert lib.pfnl_op_deinterlace_u10(*bad) == -1 and b"cur" in lib.pfnl_last_error()
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ops.deinterlace(buf[:24].view(4, 2, 3), buf[:24].view(4, 2, 3), buf[:24].view(4, 2, 3), buf[:24].view(4, 2, 3), buf[:24].view(4, 2, 3), 2)


# ---- the session ----------------------------------------------------------------------------------------------------------------------------
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


def _rgb(maxv, n=F, h=H):
    return deint_gen.woven_rgb(n, h, W, maxv, seed=11)


# name -> (the keywords of the interlaced session, those of the progressive RGB session, maxv, woven frames in the pushed layout)
def _inputs(name, n=F):
    if name == "rgb24":
        return {}, {}, 255, _rgb(255, n)
    if name == "rgb10":
        kw = {"in_depth": 10, "out_format": "rgb10"}
        return kw, kw, 1023, _rgb(1023, n)
    if name == "i420":
        return {"pixel_format": "i420"}, {"out_format": "i420"}, 255, [yuv.from_rgb(f, "i420") for f in _rgb(255, n)]
    if name == "nv12-422":
        return ({"pixel_format": "nv12", "chroma": "422", "matrix": "bt601"}, {"out_format": "nv12", "chroma": "422", "matrix": "bt601"}, 255,
                [yuv.from_rgb(f, "nv12", "bt601", False, "left", "422") for f in _rgb(255, n)])
    if name == "i420-444":
        return ({"pixel_format": "i420", "chroma": "444", "full_range": True}, {"out_format": "i420", "chroma": "444", "full_range": True}, 255,
                [yuv.from_rgb(f, "i420", "bt709", True, "left", "444") for f in _rgb(255, n)])
    if name == "yuyv422":
        return ({"pixel_format": "nv12", "chroma": "422", "packing": "yuyv422", "out_format": "rgb24", "chroma_siting": "center"}, {}, 255,
                [P.from_rgb(f, "yuyv422", "bt709", False, "center") for f in _rgb(255, n)])
    assert name == "v210"
    return ({"pixel_format": "i420", "in_depth": 10, "chroma": "422", "packing": "v210", "out_format": "i010", "out_chroma": "422"},
            {"in_depth": 10, "out_format": "i010", "out_chroma": "422"}, 1023, [P.from_rgb(f, "v210") for f in _rgb(1023, n)])


def _decode_kw(kw):
    return {"pixel_format": kw.get("pixel_format", "rgb24"), "in_depth": kw.get("in_depth", 8), "chroma": kw.get("chroma", "420"),
            "packing": kw.get("packing"), "matrix": kw.get("matrix", "bt709"), "full_range": kw.get("full_range", False),
            "siting": kw.get("chroma_siting", "left")}


def _progressive(kw, woven, maxv, order, rate, h=H):
    dk = _decode_kw(kw)
    fmt = dk.pop("pixel_format")
    return deinterlace.frames([deinterlace.decode_fields(f, fmt, h, W, **dk) for f in woven], order, rate, maxv)


def _drive(vs, frames, how="host", before=None):
    """push, pop what is ready, ... end: [(index, frame)] with host frames.  how: "host" | "device" | "alt" (the two alternating)"""
    got = []
    for i, f in enumerate(frames):
        if before:
            before(i)
        device = how == "device" or (how == "alt" and i % 2 == 1)
        got += vs.push(_cuda(np.array(f)) if device else f)
        got += vs.pop_ready()
    got += vs.end()
    return [(i, _numpy(f) if torch.is_tensor(f) else f) for i, f in got]


def _same(got, want):
    assert [i for i, _ in got] == [i for i, _ in want] == list(range(len(want)))
    for (i, a), (_, b) in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (i, int((a != b).sum()))


@pytest.mark.parametrize("rate,order", [("frame", "tff"), ("frame", "bff"), ("field", "tff"), ("field", "bff")])
@pytest.mark.parametrize("name", ["rgb24", "rgb10", "i420", "nv12-422", "i420-444", "yuyv422", "v210"])
def test_an_interlaced_session_equals_the_progressive_session_of_its_frames(engines, name, rate, order):
    kw, ref_kw, maxv, woven = _inputs(name)
    frames = _progressive(kw, woven, maxv, order, rate)
    assert len(frames) == (F if rate == "frame" else 2 * F)
    with engines[1].open_stream(H, W, BATCH, **ref_kw) as vs:
        want = _drive(vs, frames)
    with engines[0].open_stream(H, W, BATCH, interlaced=rate, field_order=order, **kw) as vs:
        assert (vs.interlaced, vs.field_order) == (rate, order)
        for how in ("host", "device", "alt"):
            _same(_drive(vs, woven, how), want)
            vs.reset()                                                   # the setting survives


def test_push_planes_from_a_pitched_surface(engines):
    kw, ref_kw, maxv, woven = _inputs("nv12-422")
    frames = _progressive(kw, woven, maxv, "tff", "field")
    with engines[1].open_stream(H, W, BATCH, **ref_kw) as vs:
        want = _drive(vs, frames)
    for device in (True, False):
        with engines[0].open_stream(H, W, BATCH, interlaced="field", **kw) as vs:
            got = []
            for f in woven:
                bufs = surface.embed(surface.split(f, "nv12", H, W, "422"), [W + 40, W + 24], 0x3C)
                bufs = [torch.from_numpy(b).cuda() for b in bufs] if device else bufs
                got += vs.push_planes(*surface.views(bufs, "nv12", H, W, "422"))
                got += vs.pop_ready()
            got += vs.end()
            _same([(i, _numpy(f) if torch.is_tensor(f) else f) for i, f in got], want)


def test_the_route_behind_the_ring_is_untouched(engines):
    kw, _, maxv, woven = _inputs("i420")
    frames = _progressive(kw, woven, maxv, "bff", "field")
    out = {"out_format": "nv12", "out_size": (48, 80)}
    with engines[1].open_stream(H, W, BATCH, **out) as vs:
        want = _drive(vs, frames)
    with engines[0].open_stream(H, W, BATCH, pixel_format="i420", interlaced="field", field_order="bff", **out) as vs:
        _same(_drive(vs, woven, "alt"), want)


@pytest.mark.parametrize("rate", ["frame", "field"])
def test_the_bound_refuses_a_push_and_changes_nothing(engines, rate):
    n = 12
    woven = _rgb(255, n)
    frames = deinterlace.frames(woven, "tff", rate)
    with engines[1].open_stream(H, W, BATCH) as vs:
        want = _drive(vs, frames)
    with engines[0].open_stream(H, W, BATCH, interlaced=rate) as vs:
        lib, s = vs._lib, vs._handle()
        push = lambda f: lib.pfnl_stream_push(s, f.ctypes.data_as(C.c_void_p), 0)   # noqa: E731
        i = 0
        while i < n and push(woven[i]) == 0:                             # no pops
            i += 1
        assert 0 < i < n and b"pop first" in lib.pfnl_last_error()
        ready = vs.ready()
        assert ready == 2 * BATCH
        assert push(woven[i]) == -2 and vs.ready() == ready              # PFNL_ERR_STATE again: the frame was not stored, no counter moved
        assert lib.pfnl_stream_end(s) == -2 and vs.ready() == ready      # the held frame does not fit either, and the session is un-ended
        got = vs.pop_ready()
        assert [k for k, _ in got] == list(range(ready))
        for f in woven[i:]:                                              # the refused frame again, and the rest: the same bytes
            got += vs.push(f)
            got += vs.pop_ready()
        got += vs.end()
        _same(got, want)


@pytest.mark.parametrize("rate", ["frame", "field"])
def test_a_mark_travels_with_its_frame(engines, rate):
    woven = _rgb(255)
    frames = deinterlace.frames(woven, "tff", rate)
    at = 3 if rate == "frame" else 6
    with engines[1].open_stream(H, W, BATCH, scene_cut="manual") as vs:
        want = _drive(vs, frames, before=lambda i: vs.mark_cut() if i == at else None)
        assert vs.cuts == [at]
    with engines[0].open_stream(H, W, BATCH, scene_cut="manual", interlaced=rate) as vs:
        for how in ("host", "device"):
            _same(_drive(vs, woven, how, before=lambda i: vs.mark_cut() if i == 3 else None), want)
            assert vs.cuts == [at]
            vs.reset()


def test_reset_in_mid_sequence(engines):
    woven = _rgb(255)
    with engines[0].open_stream(H, W, BATCH, scene_cut="manual", interlaced="field", field_order="bff") as vs:
        fresh = _drive(vs, woven)
    with engines[0].open_stream(H, W, BATCH, scene_cut="manual", interlaced="field", field_order="bff") as vs:
        vs.push(woven[3])
        vs.mark_cut()                                                    # a pending mark is forgotten
        vs.push(_cuda(woven[4]))
        vs.reset()
        _same(_drive(vs, woven), fresh)
        assert vs.cuts == []


def test_refusals(engines):
    i420, rgb24 = _capi.PIXEL_FORMATS["i420"], _capi.PIXEL_FORMATS["rgb24"]
    for bad in ({"interlaced": "both"}, {"interlaced": 1}, {"interlaced": "frame", "field_order": "top"},
                {"interlaced": "field", "pixel_format": "i420", "H": 18}):
        with pytest.raises(ValueError):                                  # refused before anything touches the engine
            engines[0].open_stream(bad.pop("H", H), W, BATCH, **bad)
    with engines[0].open_stream(H, W, BATCH) as vs:
        lib, s = vs._lib, vs._s
        assert lib.pfnl_stream_interlace(None, 1, 0) == -1
        assert lib.pfnl_stream_interlace(s, 3, 0) == -1 and lib.pfnl_stream_interlace(s, -1, 0) == -1 and lib.pfnl_stream_interlace(s, 1, 2) == -1
        vs.push(_rgb(255)[0])
        assert lib.pfnl_stream_interlace(s, 1, 0) == -2 and b"before the first frame" in lib.pfnl_last_error()
        vs.reset()
        assert lib.pfnl_stream_interlace(s, 2, 1) == 0
        vs.interlaced = "field"
        vs.push(_rgb(255)[0])                                            # held: no ring frame yet, and the settings are fixed all the same
        assert lib.pfnl_stream_interlace(s, 0, 0) == -2 and lib.pfnl_stream_ensemble(s, 2) == -2
    with engines[0].open_stream(18, W, BATCH, pixel_format="i420") as vs:   # 4:2:0 and H = 18: whichever call comes second refuses
        assert vs._lib.pfnl_stream_interlace(vs._s, 1, 0) == -1 and b"multiple of 4" in vs._lib.pfnl_last_error()
        assert vs._lib.pfnl_stream_chroma_format(vs._s, 1, 1) == 0 and vs._lib.pfnl_stream_interlace(vs._s, 1, 0) == 0
        assert vs._lib.pfnl_stream_chroma_format(vs._s, 0, 0) == -1 and b"multiple of 4" in vs._lib.pfnl_last_error()
    with engines[0].open_stream(18, W, BATCH, interlaced="frame") as vs:
        assert vs._lib.pfnl_stream_format(vs._s, i420, i420, 1, 0) == -1 and b"multiple of 4" in vs._lib.pfnl_last_error()
        assert vs._lib.pfnl_stream_format(vs._s, rgb24, i420, 1, 0) == 0
    with engines[0].open_stream(18, W, BATCH, pixel_format="i420", chroma="422", interlaced="frame") as vs:
        assert vs.interlaced == "frame"


# ---- the Y4M loop ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", ["frame", "field"])
def test_upscale_on_an_interlaced_y4m_stream_equals_the_session_driven_directly(engines, rate):
    import io

    from pfnl_amd import upscale, y4m
    woven = [yuv.from_rgb(f, "i420", "bt601", False, "left") for f in _rgb(255)]
    src = io.BytesIO()
    wr = y4m.Y4MWriter(src, y4m.Y4MHeader(W, H, "25:1", "t", (1, 1), "left", interlaced_ok=True))
    for f in woven:
        wr.write_frame(f)
    assert src.getvalue().startswith(b"YUV4MPEG2 W24 H16 F25:1 It ")
    out, log = io.BytesIO(), io.StringIO()
    reader = y4m.Y4MReader(io.BytesIO(src.getvalue()), interlaced=True)
    n = F if rate == "frame" else 2 * F
    assert upscale.upscale(reader, y4m.Y4MWriter(out), engines[0].open_stream, batch=BATCH, deinterlace=rate, log=log) == n
    with engines[1].open_stream(H, W, BATCH, pixel_format="i420", matrix="bt601", interlaced=rate, field_order="tff") as vs:
        want = _drive(vs, woven)
    back = y4m.Y4MReader(io.BytesIO(out.getvalue()))
    assert back.header.interlace == "p" and back.header.rate == ("25:1" if rate == "frame" else "50:1")
    got = list(back)
    assert len(got) == len(want) == n and all(np.array_equal(g, w_) for g, (_, w_) in zip(got, want))
    with pytest.raises(ValueError, match="It"):                          # without the keyword the loop names the tag
        upscale.upscale(y4m.Y4MReader(io.BytesIO(src.getvalue()), interlaced=True), y4m.Y4MWriter(io.BytesIO()), engines[0].open_stream)


@pytest.mark.parametrize("maxv", [255, 1023])
@pytest.mark.parametrize("h,w", [(6, 5), (8, 16), (12, 22)])
def test_the_two_frame_launch_equals_two_one_frame_launches(h, w, maxv):
    fields, parity = _fields(h, w, maxv)
    dev = [_cuda(f) for f in fields]
    got = _numpy(ops.deinterlace_pair(dev, parity[2]))
    assert got.shape == (2, h, w, 3)
    for i, k in enumerate((2, 3)):
        assert np.array_equal(got[i], deinterlace.interpolate(fields[k - 2], fields[k - 1], fields[k], fields[k + 1], fields[k + 2], parity[k], maxv))
