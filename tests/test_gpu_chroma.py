"""4:2:2 and 4:4:4 on a real MI355X (include/pfnl_hip.h CHROMA FORMAT; pfnl_amd/csrc/yuv_chroma.hip): both conversion kernels, both layouts,
both depths, and the session's two edges (pfnl_stream_chroma_format), against the host rule pfnl_amd/yuv.py / pfnl_amd/depth10.py with
chroma = "422" | "444" - byte for byte, sample for sample, no tolerance anywhere - and the Y4M loop of pfnl_amd/upscale.py against the session
driven directly."""
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfnl_amd import _capi, depth10, ops, surface, synth, y4m, yuv  # noqa: E402
from pfnl_amd import upscale as up  # noqa: E402
from pfnl_amd.engine import PFNLEngine  # noqa: E402
from pfnl_amd.spec import PFNLGeometry  # noqa: E402

PAIRS = [("bt601", False), ("bt709", True)]
# what of a siting each subsampling reads: the horizontal axis at 4:2:2 (co-sited | midway), nothing at 4:4:4
CASES = [("422", "left"), ("422", "center"), ("444", "left")]
# 4:2:2, 8 bits: (1, 2) nothing but edges; (3, 6); (5, 34) single bytes, W / 2 odd; (4, 36) 4-byte words; (2, 64) 16-byte words; (3, 66)
# 4:4:4, 8 bits: (1, 1); (3, 5) odd width; (2, 36) 4-byte words; (2, 64) 16-byte words; (3, 65) more than one strip of single bytes
SHAPES = {"422": [(1, 2), (3, 6), (5, 34), (4, 36), (2, 64), (3, 66)], "444": [(1, 1), (3, 5), (2, 36), (2, 64), (3, 65)]}
SHAPES10 = {"422": [(1, 2), (3, 10), (2, 64)], "444": [(1, 1), (3, 10), (2, 64)]}   # edges; single samples; 16-byte words
H, W, BATCH, F = 16, 24, 2, 5                                           # the sessions: one block, sH x sW = 64 x 96
DEPTHS = {8: (yuv.FORMATS, 256, np.uint8), 10: (depth10.FORMATS, 1024, np.uint16)}


def _params(shapes):
    return [pytest.param(c, s, h, w, id=f"{c}-{s}-{h}x{w}") for c, s in CASES for h, w in shapes[c]]


def _with_all_values(rng, shape, levels):
    a = rng.integers(0, levels, size=shape).astype(np.uint16 if levels > 256 else np.uint8)
    flat = a.reshape(-1)
    if flat.size >= levels:
        flat[rng.permutation(flat.size)[:levels]] = np.arange(levels)
        assert len(np.unique(flat)) == levels
    return a


def _extreme_blocks(rng, shape, top, block=2):
    """0 or ``top`` in blocks of ``block`` samples: every clip of either direction fires next to its opposite"""
    small = rng.integers(0, 2, size=tuple((s + block - 1) // block for s in shape[:2]) + tuple(shape[2:])) * top
    return np.repeat(np.repeat(small, block, axis=0), block, axis=1)[:shape[0], :shape[1]].astype(np.uint16 if top > 255 else np.uint8)


def _host(bits):
    """(pack, to_rgb, from_rgb) of the depth"""
    return (yuv.pack, yuv.to_rgb, yuv.from_rgb) if bits == 8 else (depth10.pack10, depth10.to_rgb10, depth10.from_rgb10)


def _yuv_frames(n, h, w, fmt, chroma, seed, bits=8):
    """n packed frames [n, rows, w] of valid samples: random planes that hold every value where they can, the last one 0 / max blocks"""
    levels = DEPTHS[bits][1]
    rng = np.random.default_rng(seed)
    cs = yuv.chroma_shape(h, w, chroma)
    planes = [[_with_all_values(rng, s, levels) for s in ((h, w), cs, cs)] for _ in range(n)]
    if n > 1:
        planes[-1] = [_extreme_blocks(rng, s, levels - 1) for s in ((h, w), cs, cs)]
    return np.stack([_host(bits)[0](*p, fmt, chroma) for p in planes])


def _rgb_frames(n, h, w, seed, bits=8):
    levels = DEPTHS[bits][1]
    rng = np.random.default_rng(seed)
    frames = [_with_all_values(rng, (h, w, 3), levels) for _ in range(n)]
    if n > 1:
        frames[-1] = _extreme_blocks(rng, (h, w, 3), levels - 1)
    return np.stack(frames)


def _decode_op(bits):
    return ops.yuv_to_rgb if bits == 8 else ops.yuv_to_rgb_u10


def _encode_op(bits):
    return ops.rgb_to_yuv if bits == 8 else ops.rgb_to_yuv_u10


def _check_decode(bits, chroma, siting, h, w):
    formats, levels, dtype = DEPTHS[bits]
    for fmt in formats:
        for n in (1, 3):
            frames = _yuv_frames(n, h, w, fmt, chroma, seed=h * 1000 + w + n, bits=bits)
            dev = torch.from_numpy(frames).cuda()
            for matrix, full in PAIRS:
                got = _decode_op(bits)(dev, fmt, h, w, matrix, full, chroma=chroma, siting=siting).cpu().numpy()
                want = np.stack([_host(bits)[1](f, fmt, h, w, matrix, full, siting=siting, chroma=chroma) for f in frames])
                assert got.dtype == dtype and got.shape == want.shape == (n, h, w, 3)
                assert np.array_equal(got, want), (bits, h, w, fmt, chroma, siting, n, matrix, full, int((got != want).sum()))
                if n > 1 and h * w >= 128:
                    assert want[-1].min() == 0 and want[-1].max() == levels - 1               # the extreme planes clip at both ends


def _check_encode(bits, chroma, siting, h, w):
    formats, _, dtype = DEPTHS[bits]
    for fmt in formats:
        for n in (1, 3):
            frames = _rgb_frames(n, h, w, seed=h * 1000 + w + 10 + n, bits=bits)
            dev = torch.from_numpy(frames).cuda()
            for matrix, full in PAIRS:
                got = _encode_op(bits)(dev, fmt, matrix, full, chroma=chroma, siting=siting).cpu().numpy()
                want = np.stack([_host(bits)[2](f, fmt, matrix, full, siting=siting, chroma=chroma) for f in frames])
                assert got.dtype == dtype and got.shape == want.shape == (n, yuv.frame_bytes(h, w, chroma) // w, w)
                assert np.array_equal(got, want), (bits, h, w, fmt, chroma, siting, n, matrix, full, int((got != want).sum()))


# ---- the ops ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chroma,siting,h,w", _params(SHAPES))
def test_decode_equals_the_host_rule(chroma, siting, h, w):
    _check_decode(8, chroma, siting, h, w)


@pytest.mark.parametrize("chroma,siting,h,w", _params(SHAPES))
def test_encode_equals_the_host_rule(chroma, siting, h, w):
    _check_encode(8, chroma, siting, h, w)


@pytest.mark.parametrize("chroma,siting,h,w", _params(SHAPES10))
def test_10_bit_decode_equals_the_host_rule(chroma, siting, h, w):
    _check_decode(10, chroma, siting, h, w)


@pytest.mark.parametrize("chroma,siting,h,w", _params(SHAPES10))
def test_10_bit_encode_equals_the_host_rule(chroma, siting, h, w):
    _check_encode(10, chroma, siting, h, w)


def test_the_siting_is_read_for_its_horizontal_axis_alone():
    """4:2:2: "topleft" is "left"; 4:4:4: every siting is the same conversion - on the device as in the rule"""
    h, w = 4, 36
    for chroma, same in (("422", ("left", "topleft")), ("444", yuv.SITINGS)):
        for fmt in yuv.FORMATS:
            frames = torch.from_numpy(_yuv_frames(2, h, w, fmt, chroma, seed=3)).cuda()
            rgbs = torch.from_numpy(_rgb_frames(2, h, w, seed=4)).cuda()
            dec = [ops.yuv_to_rgb(frames, fmt, h, w, "bt709", False, chroma=chroma, siting=s).cpu().numpy() for s in same]
            enc = [ops.rgb_to_yuv(rgbs, fmt, "bt709", False, chroma=chroma, siting=s).cpu().numpy() for s in same]
            assert all(np.array_equal(d, dec[0]) for d in dec) and all(np.array_equal(e, enc[0]) for e in enc), (chroma, fmt)


def test_chroma_420_is_the_sited_hook():
    h, w = 4, 36
    for fmt in yuv.FORMATS:
        frames = torch.from_numpy(_yuv_frames(2, h, w, fmt, "420", seed=8)).cuda()
        rgbs = torch.from_numpy(_rgb_frames(2, h, w, seed=9)).cuda()
        for siting in yuv.SITINGS:
            assert torch.equal(ops.yuv_to_rgb(frames, fmt, h, w, siting=siting), ops.yuv420_to_rgb(frames, fmt, h, w, siting=siting))
            assert torch.equal(ops.rgb_to_yuv(rgbs, fmt, siting=siting), ops.rgb_to_yuv420(rgbs, fmt, siting=siting))


def _guarded(op, src_np, out_samples, off, slack=64):
    """runs op(src, out) with both tensors ``off`` samples behind a 16-byte boundary and a pattern on both sides of the destination:
    (what the destination holds, whether the pattern is intact)"""
    dtype, sz = src_np.dtype, src_np.dtype.itemsize
    raw, tdt = (np.uint8, torch.uint8) if sz == 1 else (np.int16, torch.uint16)          # (torch fills and copies int16, not uint16)
    pattern = ((np.arange(slack + off + out_samples + slack) * 7 + 3) % (1 << (8 * sz))).astype(dtype)
    src = torch.zeros(off + src_np.size, dtype=torch.uint8 if sz == 1 else torch.int16, device="cuda")
    src[off:] = torch.from_numpy(src_np.reshape(-1).view(raw)).cuda()
    dst = torch.from_numpy(pattern.view(raw)).cuda().view(tdt)
    lo = slack + off
    assert (src.data_ptr() + sz * off) % 16 == (sz * off) % 16 and (dst.data_ptr() + sz * lo) % 16 == (sz * off) % 16
    op(src.view(tdt)[off:], dst[lo:lo + out_samples])
    got = dst.view(torch.uint8 if sz == 1 else torch.int16).cpu().numpy().view(dtype)
    return got[lo:lo + out_samples], np.array_equal(got[:lo], pattern[:lo]) and np.array_equal(got[lo + out_samples:], pattern[lo + out_samples:])


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("chroma,siting", CASES)
def test_unaligned_pointers_take_a_narrower_form_and_stay_inside_the_destination(chroma, siting, bits):
    """shapes whose aligned form uses words; at a pointer that is off by 1 or 4 bytes (16 bits: by one sample) it must not"""
    formats = DEPTHS[bits][0]
    n = 2
    for h, w in ([(2, 64), (4, 36)] if bits == 8 else [(2, 64)]):
        ys, rs = n * yuv.frame_bytes(h, w, chroma), n * h * w * 3               # samples
        for fmt in formats:
            frames = _yuv_frames(n, h, w, fmt, chroma, seed=5, bits=bits)
            rgbs = _rgb_frames(n, h, w, seed=6, bits=bits)
            for off in ((1, 4) if bits == 8 else (1,)):                        # in samples: 1 | 4 bytes, or one 16-bit sample
                got, intact = _guarded(lambda x, out: _decode_op(bits)(x, fmt, h, w, "bt601", False, chroma=chroma, siting=siting, out=out),
                                       frames, rs, off)
                want = np.stack([_host(bits)[1](f, fmt, h, w, "bt601", False, siting=siting, chroma=chroma) for f in frames])
                assert np.array_equal(got.reshape(want.shape), want) and intact, (fmt, h, w, off, intact)
                got, intact = _guarded(lambda x, out: _encode_op(bits)(x.view(n, h, w, 3), fmt, "bt601", False, chroma=chroma, siting=siting,
                                                                       out=out), rgbs, ys, off)
                want = np.stack([_host(bits)[2](f, fmt, "bt601", False, siting=siting, chroma=chroma) for f in rgbs])
                assert np.array_equal(got.reshape(want.shape), want) and intact, (fmt, h, w, off, intact)


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("chroma,siting", CASES)
def test_surface_decode_on_pitched_planes_equals_the_packed_decode(chroma, siting, bits):
    formats, _, dtype = DEPTHS[bits]
    op = ops.yuv_to_rgb_surface if bits == 8 else ops.yuv_to_rgb_surface_u10
    sz = np.dtype(dtype).itemsize
    for h, w in ((5, 34), (2, 64)):                                             # single samples; words where the pitch allows
        for fmt in formats:
            for frame in _yuv_frames(2, h, w, fmt, chroma, seed=77, bits=bits):
                planes = surface.split(frame, fmt, h, w, chroma)
                rows = [p.shape[1] * sz for p in planes]
                for pitches in ([r + sz for r in rows], [(r + 63) // 64 * 64 + 64 for r in rows]):
                    outs = []
                    for fill in (0x00, 0xFF):                                   # what lies between a row's end and the pitch never counts
                        bufs = [torch.from_numpy(b).cuda() for b in surface.embed(planes, pitches, fill)]
                        views = surface.views(bufs, fmt, h, w, chroma)
                        assert surface.describe(views, fmt, h, w, chroma)[1] == pitches
                        outs.append(op(views, fmt, h, w, "bt709", False, chroma=chroma, siting=siting).cpu().numpy())
                        for b, p, r in zip(bufs, planes, rows):                 # the surface itself is only read
                            assert (b.cpu().numpy()[:, r:] == fill).all()
                    want = _host(bits)[1](frame, fmt, h, w, "bt709", False, siting=siting, chroma=chroma)
                    assert np.array_equal(outs[0], want) and np.array_equal(outs[1], want), (bits, fmt, chroma, siting, pitches)


@pytest.mark.parametrize("chroma,siting", CASES)
def test_a_window_of_a_larger_surface_is_the_frame(chroma, siting):
    """plane pointers at the window's first sample, the surface's pitch kept: chroma clamps at the window's edges, not the surface's"""
    H, W, h, w, y0, x0 = 12, 96, 5, 34, 3, 18
    rng = np.random.default_rng(11)
    for fmt in yuv.FORMATS:
        big = [torch.from_numpy(rng.integers(0, 256, size=(r, n), dtype=np.uint8)).cuda() for r, n, _ in surface.plane_shapes(fmt, H, W, chroma)]
        cx = x0 if chroma == "444" else x0 // 2                                 # the window's first chroma sample of a row
        if fmt == "nv12":
            views = [big[0][y0:y0 + h, x0:x0 + w], big[1][y0:y0 + h, 2 * cx:2 * cx + surface.plane_shapes(fmt, h, w, chroma)[1][1]]]
        else:
            cw = surface.plane_shapes(fmt, h, w, chroma)[1][1]
            views = [big[0][y0:y0 + h, x0:x0 + w], big[1][y0:y0 + h, cx:cx + cw], big[2][y0:y0 + h, cx:cx + cw]]
        frame = np.concatenate([v.cpu().numpy().reshape(-1) for v in views])
        got = ops.yuv_to_rgb_surface(views, fmt, h, w, "bt601", True, chroma=chroma, siting=siting).cpu().numpy()
        assert np.array_equal(got, yuv.to_rgb(frame, fmt, h, w, "bt601", True, siting=siting, chroma=chroma)), (fmt, chroma, siting)


# ---- the session --------------------------------------------------------------------------------------------------------------------------
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
        if device:                                                              # (torch copies int16, not uint16)
            f = np.array(f)                                                     # (a reference frame is read-only)
            f = torch.from_numpy(f).cuda() if f.dtype == np.uint8 else torch.from_numpy(f.view(np.int16)).cuda().view(torch.uint16)
        got += vs.push(f)
        got += vs.pop_ready()
    got += vs.end()
    got = [(i, (f.cpu().numpy() if f.dtype == torch.uint8 else f.view(torch.int16).cpu().numpy().view(np.uint16)) if torch.is_tensor(f) else f)
           for i, f in got]
    assert [i for i, _ in got] == list(range(len(frames)))
    return np.stack([f for _, f in got])


def _rgb_session(engine, rgb, bits, out_bits=None, **kw):
    """the SR frames of RGB frames through the session without a YUV edge: rgb24 in and out; at 10 bits values 0 .. 1023 in, and rgb10 out
    unless ``out_bits`` says 8"""
    depth = {"in_depth": 10} if bits == 10 else {}
    if (out_bits or bits) == 10:
        depth["out_format"] = "rgb10"
    with engine.open_stream(H, W, BATCH, **depth, **kw) as vs:
        return _stream_all(vs, list(rgb))


def _names(bits, layout):
    """(pixel_format, the name of the layout among the depth's formats, in_depth keywords, the out_format of that layout)"""
    fmt = layout if bits == 8 else {"nv12": "p010", "i420": "i010"}[layout]
    return layout, fmt, ({} if bits == 8 else {"in_depth": 10}), fmt


@pytest.fixture(scope="module")
def rgb_reference(engines):
    """per depth (the RGB frames, their SR frames out of the RGB session): computed once, read by the output tests"""
    out = {}
    for bits in (8, 10):
        rgb = _rgb_frames(F, H, W, seed=40 + bits, bits=bits)
        sr = _rgb_session(engines[1], rgb, bits)
        rgb.setflags(write=False), sr.setflags(write=False)
        out[bits] = (rgb, sr)
    return out


IN_CASES = [(8, "422", "i420", "left"), (8, "444", "nv12", "left"), (10, "422", "nv12", "center"), (10, "444", "i420", "left")]


@pytest.mark.parametrize("bits,chroma,layout,siting", IN_CASES)
def test_input_at_the_new_subsamplings_equals_the_rgb_session_fed_the_host_decode(engines, bits, chroma, layout, siting):
    pix, fmt, depth, _ = _names(bits, layout)
    frames = list(_yuv_frames(F, H, W, fmt, chroma, seed=50 + bits, bits=bits))
    rgb = [_host(bits)[1](f, fmt, H, W, "bt601", False, siting=siting, chroma=chroma) for f in frames]
    want = _rgb_session(engines[1], rgb, bits, out_bits=8)
    with engines[0].open_stream(H, W, BATCH, pixel_format=pix, out_format="rgb24", matrix="bt601", chroma=chroma, chroma_siting=siting,
                                **depth) as vs:
        assert (vs.chroma, vs.out_chroma) == (chroma, chroma)
        for device in (False, True):
            got = _stream_all(vs, frames, device)
            assert got.shape == (F, 4 * H, 4 * W, 3) and got.dtype == np.uint8 and np.array_equal(got, want), (device, int((got != want).sum()))
            vs.reset()                                                          # the subsampling survives
    if bits == 10:                                                             # 10 bits end to end: out in the same layout, against the host encode
        want10 = np.stack([_host(10)[2](f, fmt, "bt601", False, siting=siting, chroma=chroma) for f in _rgb_session(engines[1], rgb, 10)])
        with engines[0].open_stream(H, W, BATCH, pixel_format=pix, out_format=fmt, matrix="bt601", chroma=chroma, chroma_siting=siting,
                                    **depth) as vs:
            for device in (False, True):
                got = _stream_all(vs, frames, device)
                assert got.dtype == np.uint16 and np.array_equal(got, want10), (device, int((got != want10).sum()))
                vs.reset()


OUT_CASES = [(8, "422", "nv12", "left"), (8, "444", "i420", "left"), (10, "422", "i420", "center"), (10, "444", "nv12", "left")]


@pytest.mark.parametrize("bits,chroma,layout,siting", OUT_CASES)
def test_output_at_the_new_subsamplings_equals_the_host_encode_of_the_rgb_sessions_frames(engines, rgb_reference, bits, chroma, layout, siting):
    _, fmt, _, out_format = _names(bits, layout)
    rgb, sr = rgb_reference[bits]
    want = np.stack([_host(bits)[2](f, fmt, "bt709", False, siting=siting, chroma=chroma) for f in sr])
    depth = {} if bits == 8 else {"in_depth": 10}
    with engines[0].open_stream(H, W, BATCH, out_format=out_format, out_chroma=chroma, out_chroma_siting=siting, **depth) as vs:
        assert (vs.chroma, vs.out_chroma) == ("420", chroma)
        for device in (False, True):
            got = _stream_all(vs, list(rgb), device)
            assert got.shape == (F, yuv.frame_bytes(4 * H, 4 * W, chroma) // (4 * W), 4 * W) and got.dtype == want.dtype
            assert np.array_equal(got, want), (device, int((got != want).sum()))
            vs.reset()


@pytest.mark.parametrize("chroma,out_size", [("422", (63, 96)), ("444", (63, 95))])
def test_an_output_size_that_only_the_new_subsampling_allows(engines, rgb_reference, chroma, out_size):
    rgb, _ = rgb_reference[8]
    sr = _rgb_session(engines[1], rgb, 8, out_size=out_size)
    want = np.stack([yuv.from_rgb(f, "i420", chroma=chroma) for f in sr])
    with engines[0].open_stream(H, W, BATCH, out_format="i420", out_chroma=chroma, out_size=out_size) as vs:
        got = _stream_all(vs, list(rgb))
        assert got.shape == want.shape == (F, yuv.frame_bytes(*out_size, chroma) // out_size[1], out_size[1]) and np.array_equal(got, want)
    for tighter in {"422": ("420",), "444": ("420", "422")}[chroma]:            # refused before anything touches the engine
        with pytest.raises(ValueError):
            engines[0].open_stream(H, W, BATCH, out_format="i420", out_chroma=tighter, out_size=out_size)


def test_fit_contain_on_a_422_canvas(engines, rgb_reference):
    rgb, _ = rgb_reference[8]
    with engines[0].open_stream(H, W, BATCH, out_format="nv12", out_chroma="422", out_size=(45, 90), fit="contain", fill=(16, 128, 240)) as vs:
        assert vs.place[3] % 2 == 0 and vs.place[1] % 2 == 0                    # the grid is (1, 2): even across, anything down
        crop, place = vs.crop, vs.place
        got = _stream_all(vs, list(rgb))
    sr = _rgb_session(engines[1], rgb, 8, out_size=(45, 90), crop=crop, place=place, fill=(16, 128, 240))
    want = np.stack([yuv.from_rgb(f, "nv12", chroma="422") for f in sr])
    assert np.array_equal(got, want)


def test_planes_on_pitched_host_surfaces_follow_the_subsampling(engines):
    """push_planes of pitched NV16 host surfaces and pop_planes into one: the samples are from_rgb of the RGB session's frames for to_rgb of the
    input, and nothing else of the destination is written."""
    chroma, oH, oW = "422", 4 * H, 4 * W
    frames = list(_yuv_frames(F, H, W, "nv12", chroma, seed=61))
    sr = _rgb_session(engines[1], [yuv.to_rgb(f, "nv12", H, W, chroma=chroma) for f in frames], 8)
    want = [yuv.from_rgb(f, "nv12", chroma=chroma) for f in sr]
    got = []
    with engines[0].open_stream(H, W, BATCH, pixel_format="nv12", chroma=chroma) as vs:
        def drain():
            while vs.ready():
                bufs = [np.full((oH, pitch), 0xA5, np.uint8) for pitch in (oW + 64, oW + 32)]
                assert vs.pop_planes(*surface.views(bufs, "nv12", oH, oW, chroma)) == len(got)
                assert all((b[:, oW:] == 0xA5).all() for b in bufs)
                got.append(np.concatenate([bufs[0][:, :oW], bufs[1][:, :oW]]))

        for f in frames:
            bufs = surface.embed(surface.split(f, "nv12", H, W, chroma), [W + 40, W + 8], 0x3C)
            assert vs.push_planes(*surface.views(bufs, "nv12", H, W, chroma)) == []
            drain()
        vs._lib.pfnl_stream_end(vs._handle())
        drain()
    assert len(got) == F and all(np.array_equal(g, w_) for g, w_ in zip(got, want))


def test_setter_order_and_a_refused_call(engines):
    """pfnl_stream_chroma_format before and after pfnl_stream_format gives the same bytes; a refused call leaves the session delivering what
    it delivered"""
    frames = list(_yuv_frames(F, H, W, "i420", "422", seed=62))
    i420 = _capi.PIXEL_FORMATS["i420"]
    outs = []
    for chroma_first in (True, False):
        with engines[0].open_stream(H, W, BATCH) as vs:
            lib, s = vs._lib, vs._s
            calls = [lambda: lib.pfnl_stream_chroma_format(s, 1, 2), lambda: lib.pfnl_stream_format(s, i420, i420, 1, 0)]
            for call in (calls if chroma_first else calls[::-1]):
                assert call() == 0, lib.pfnl_last_error()
            vs.pixel_format = vs.out_format = "i420"                            # (what the keywords would have noted)
            vs.chroma, vs.out_chroma = "422", "444"
            outs.append(_stream_all(vs, frames))
            vs.reset()
            assert lib.pfnl_stream_chroma_format(s, 3, 0) == -1 and b"chroma format" in lib.pfnl_last_error()
            assert lib.pfnl_stream_chroma_format(s, 0, -1) == -1
            assert lib.pfnl_stream_resize(s, 63, 95) == 0                       # legal at 4:4:4 out alone:
            assert lib.pfnl_stream_chroma_format(s, 1, 1) == -1 and b"even" in lib.pfnl_last_error()   # 4:2:2 needs an even width,
            assert lib.pfnl_stream_chroma_format(s, 1, 0) == -1 and b"even" in lib.pfnl_last_error()   # 4:2:0 an even size
            assert lib.pfnl_stream_resize(s, 0, 0) == 0
            assert np.array_equal(_stream_all(vs, frames), outs[-1])           # in 4:2:2, out 4:4:4 as before
            vs.reset()
            vs.push(frames[0])
            assert lib.pfnl_stream_chroma_format(s, 0, 0) == -2 and b"before the first frame" in lib.pfnl_last_error()   # PFNL_ERR_STATE
    assert outs[0].shape == (F, 3 * 4 * H, 4 * W) and np.array_equal(outs[0], outs[1])
    with engines[1].open_stream(H, W, BATCH, pixel_format="i420", chroma="422", out_chroma="444") as vs:
        assert np.array_equal(_stream_all(vs, frames), outs[0])
    for bad in ({"chroma": "4:2:2"}, {"out_chroma": 1}):                        # refused before anything touches the engine
        with pytest.raises(ValueError):
            engines[0].open_stream(H, W, BATCH, pixel_format="i420", **bad)


# ---- Y4M end to end -------------------------------------------------------------------------------------------------------------------------
def test_upscale_of_422_and_444p10_streams_equals_the_session_driven_directly(engines):
    for tag, chroma, bits, kw, out_tag in ((b"C422", "422", 8, {}, b"C422 XYSCSS=422"),
                                           (b"C444p10 XYSCSS=444P10", "444", 10, {"out_format": "i010"}, b"C444p10 XYSCSS=444P10")):
        fmt = "i420" if bits == 8 else "i010"
        frames = list(_yuv_frames(F, H, W, fmt, chroma, seed=70 + bits, bits=bits))
        data = b"YUV4MPEG2 W24 H16 F25:1 Ip A1:1 " + tag + b"\n" + b"".join(b"FRAME\n" + f.astype("<u2" if bits == 10 else np.uint8).tobytes()
                                                                             for f in frames)
        with pytest.raises(ValueError, match="C4"):                            # without the opt-in the tag is refused by name
            y4m.Y4MReader(io.BytesIO(data), depths=(8, 10))
        out, log = io.BytesIO(), io.StringIO()
        reader = y4m.Y4MReader(io.BytesIO(data), depths=(8, 10), chromas=y4m.CHROMAS)
        assert up.upscale(reader, y4m.Y4MWriter(out), engines[0].open_stream, batch=BATCH, log=log, **kw) == F
        depth = {} if bits == 8 else {"in_depth": 10}
        with engines[1].open_stream(H, W, BATCH, pixel_format="i420", out_format=fmt, matrix="bt601", full_range=False, chroma=chroma,
                                    chroma_siting="left", **depth) as vs:
            want = _stream_all(vs, frames)
        head, body = out.getvalue().split(b"\n", 1)
        assert head == b"YUV4MPEG2 W96 H64 F25:1 Ip A1:1 " + out_tag
        assert body == b"".join(b"FRAME\n" + f.astype("<u2" if bits == 10 else np.uint8).tobytes() for f in want)
