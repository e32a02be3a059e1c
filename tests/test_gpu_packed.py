"""Packed formats on a real MI355X (include/pfnl_hip.h PACKED FORMATS; pfnl_amd/csrc/packed.hip): both kernels for every packing, in the
wide and the narrow form, on tight frames, offset pointers and pitched planes, and the session's two edges (pfnl_stream_packing), against
the host rule pfnl_amd/packed.py - unpack, then the planar 4:2:2 rule the project already pins - byte for byte, no tolerance anywhere; and
the raw pipe of pfnl_amd/rawvideo.py against the session driven directly."""
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfnl_amd import _capi, depth10, ops, rawvideo, surface, synth, yuv  # noqa: E402
from pfnl_amd import packed as P  # noqa: E402
from pfnl_amd.engine import PFNLEngine  # noqa: E402
from pfnl_amd.spec import PFNLGeometry  # noqa: E402

PAIRS = [("bt601", False), ("bt709", True)]
RGBA_SHAPES = [(1, 1), (3, 5), (2, 4), (2, 36), (3, 67)]                 # edges; odd; one word; words; words + tail (at a pitch on 16 bytes)
SHAPES = {
    "rgba": RGBA_SHAPES, "bgra": RGBA_SHAPES, "x2rgb10": RGBA_SHAPES, "x2bgr10": RGBA_SHAPES,
    "bgr24": [(1, 1), (3, 5), (2, 16), (3, 37)],                         # (2, 16): three words
    "yuyv422": [(1, 2), (3, 6), (2, 16), (5, 34), (2, 64), (3, 66)],     # edges only; W/2 odd; words; word + tail unit
    "uyvy422": [(1, 2), (3, 6), (2, 16), (5, 34), (2, 64), (3, 66)],
    "y210": [(1, 2), (3, 10), (2, 64), (3, 66)],
    "v210": [(1, 6), (3, 12), (2, 48), (3, 54), (2, 96)],                # one group; a full 128-byte row; a row padded 144 -> 256
}
CASES = [pytest.param(name, h, w, id=f"{name}-{h}x{w}") for name in P.PACKINGS[1:] for h, w in SHAPES[name]]
H, W, BATCH, F = 16, 24, 2, 5                                            # the sessions: one block, sH x sW = 64 x 96


def _sitings(name):
    return ("left", "center") if P.is_yuv(name) else ("left",)


def _unit(name):
    return 16 if name == "v210" else 4                                   # what an offset pointer is off by: 4 bytes, or one v210 group


def _levels(name):
    return 1 << P.bits(name)


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


def _rgb_frames(n, h, w, seed, levels=256):
    rng = np.random.default_rng(seed)
    frames = [_with_all_values(rng, (h, w, 3), levels) for _ in range(n)]
    if n > 1:
        frames[-1] = _extreme_blocks(rng, (h, w, 3), levels - 1)
    return np.stack(frames)


def _planes(n, h, w, seed, levels=256):
    """n frames as (Y, Cb, Cr) of a 4:2:2 frame: random planes that hold every value where they can, the last frame 0 / max blocks"""
    rng = np.random.default_rng(seed)
    shapes = ((h, w), (h, w // 2), (h, w // 2))
    out = [tuple(_with_all_values(rng, s, levels) for s in shapes) for _ in range(n)]
    if n > 1:
        out[-1] = tuple(_extreme_blocks(rng, s, levels - 1) for s in shapes)
    return out


def _packed_frames(name, n, h, w, seed):
    """n tight frames [n, h, tight row bytes] uint8 in the packing"""
    if P.is_yuv(name):
        return np.stack([P.pack(p, name, h, w) for p in _planes(n, h, w, seed, _levels(name))])
    return np.stack([P.pack(f, name, h, w) for f in _rgb_frames(n, h, w, seed, _levels(name))])


def _cuda(a):
    a = np.ascontiguousarray(a)                                          # (torch copies int16, not uint16)
    return torch.from_numpy(a).cuda() if a.dtype == np.uint8 else torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)


def _numpy(t):
    return t.cpu().numpy() if t.dtype == torch.uint8 else t.view(torch.int16).cpu().numpy().view(np.uint16)


def _pitched(frames, name, h, w, pitch, fill):
    """the rows of tight frames [n, h, tight] at ``pitch``, ``fill`` behind a row's samples: [n, h, pitch] uint8"""
    row = P.row_bytes(name, w)
    out = np.full((frames.shape[0], h, pitch), fill, np.uint8)
    out[:, :, :row] = frames[:, :, :row]
    return out


def _offset(a, off, fill=0x5A):
    """(a device buffer of ``fill`` with ``a``'s bytes ``off`` bytes behind a 256-byte boundary, the view of those bytes)"""
    buf = torch.full((off + a.size + 64,), fill, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    view = buf[off:off + a.size]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda())
    return buf, view


# ---- the ops --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,h,w", CASES)
def test_decode_equals_the_host_rule(name, h, w):
    row, tight, levels = P.row_bytes(name, w), P.tight_row_bytes(name, w), _levels(name)
    pitch = (row + 15) // 16 * 16 + 16                                   # rows on 16 bytes: strips of 16-byte words, and the row's tail
    for siting in _sitings(name):
        for n in (1, 3):
            frames = _packed_frames(name, n, h, w, seed=h * 1000 + w + n)
            assert frames.shape == (n, h, tight)
            dev = torch.from_numpy(frames).cuda()
            for matrix, full in PAIRS:
                want = np.stack([P.to_rgb(f, name, h, w, matrix, full, siting) for f in frames])
                got = _numpy(ops.packed_to_rgb(dev, name, h, w, matrix, full, siting))
                assert got.dtype == want.dtype and got.shape == want.shape == (n, h, w, 3)
                assert np.array_equal(got, want), (name, h, w, siting, n, matrix, full, int((got != want).sum()))
                if n > 1 and P.is_yuv(name) and h * w >= 128:
                    assert want[-1].min() == 0 and want[-1].max() == levels - 1          # the extreme planes clip at both ends
        # once from a pointer that is off by one unit: the narrow form on the same data
        matrix, full = PAIRS[0]
        _, view = _offset(frames, _unit(name))
        assert view.data_ptr() % 16 == _unit(name) % 16
        got = _numpy(ops.packed_to_rgb(view, name, h, w, matrix, full, siting))
        want = np.stack([P.to_rgb(f, name, h, w, matrix, full, siting) for f in frames])
        assert np.array_equal(got, want), (name, h, w, siting, "offset", int((got != want).sum()))
        # once at a pitch above the row: what lies behind a row's samples never counts, and is only read past
        for fill in (0x00, 0xFF):
            dev = torch.from_numpy(_pitched(frames, name, h, w, pitch, fill)).cuda()
            got = _numpy(ops.packed_to_rgb(dev, name, h, w, matrix, full, siting, pitch=pitch))
            assert np.array_equal(got, want), (name, h, w, siting, "pitch", fill, int((got != want).sum()))


@pytest.mark.parametrize("name,h,w", CASES)
def test_encode_equals_the_host_rule(name, h, w):
    row, tight, levels = P.row_bytes(name, w), P.tight_row_bytes(name, w), _levels(name)
    pitch = (row + 15) // 16 * 16 + 16
    for siting in _sitings(name):
        for n in (1, 3):
            rgb = _rgb_frames(n, h, w, seed=h * 1000 + w + 10 + n, levels=levels)
            dev = _cuda(rgb)
            for matrix, full in PAIRS:
                want = np.stack([P.from_rgb(f, name, matrix, full, siting) for f in rgb])
                got = ops.rgb_to_packed(dev, name, matrix, full, siting).cpu().numpy()
                assert got.dtype == np.uint8 and got.shape == want.shape == (n, h, tight)
                assert np.array_equal(got, want), (name, h, w, siting, n, matrix, full, int((got != want).sum()))
                assert not got[:, :, row:].any()                                         # a tight v210 row's padding reads 0
        matrix, full = PAIRS[0]
        want = np.stack([P.from_rgb(f, name, matrix, full, siting) for f in rgb])
        # once into a pointer that is off by one unit, a pattern on both sides of the destination
        off = _unit(name)
        buf, view = _offset(np.full(want.size, 0x5A, np.uint8), off)
        if tight != row:                                                                 # (the padding of a tight v210 row is the caller's 0)
            view.zero_()
        ops.rgb_to_packed(dev, name, matrix, full, siting, out=view)
        got = buf.cpu().numpy()
        assert np.array_equal(got[off:off + want.size].reshape(want.shape), want), (name, h, w, siting, "offset")
        assert (got[:off] == 0x5A).all() and (got[off + want.size:] == 0x5A).all()
        # once at a pitch above the row, sentinel bytes in the padding: encode leaves them untouched
        out = torch.full((n, h, pitch), 0xA5, dtype=torch.uint8, device="cuda")
        got = ops.rgb_to_packed(dev, name, matrix, full, siting, pitch=pitch, out=out).cpu().numpy()
        assert np.array_equal(got[:, :, :row], want[:, :, :row]), (name, h, w, siting, "pitch")
        assert (got[:, :, row:] == 0xA5).all()


def test_the_hooks_refuse_what_the_table_refuses():
    rgb8, rgb10 = torch.zeros((1, 2, 6, 3), dtype=torch.uint8, device="cuda"), torch.zeros((1, 2, 6, 3), dtype=torch.uint16, device="cuda")
    with pytest.raises(TypeError):
        ops.rgb_to_packed(rgb8, "v210")                                  # the depth follows the packing
    with pytest.raises(TypeError):
        ops.rgb_to_packed(rgb10, "yuyv422")
    with pytest.raises(ValueError, match="multiple of 6"):
        ops.rgb_to_packed(torch.zeros((1, 2, 8, 3), dtype=torch.uint16, device="cuda"), "v210")
    with pytest.raises(ValueError, match="even width"):
        ops.rgb_to_packed(torch.zeros((1, 2, 5, 3), dtype=torch.uint8, device="cuda"), "uyvy422")
    with pytest.raises(ValueError, match="pitch"):
        ops.rgb_to_packed(rgb8, "bgra", pitch=20)
    lib = _capi.load_library()
    buf = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    assert lib.pfnl_op_packed_to_rgb_u10(p + 2, 24, _capi.PACKINGS["x2rgb10"], 1, 0, 0, 1, 0, 2, 6, p + 512, None) == -1
    assert b"multiples of" in lib.pfnl_last_error()
    assert lib.pfnl_op_packed_to_rgb_u10(p, 26, _capi.PACKINGS["x2rgb10"], 1, 0, 0, 1, 0, 2, 6, p + 512, None) == -1
    assert lib.pfnl_op_packed_to_rgb_u10(p + 2, 24, _capi.PACKINGS["y210"], 1, 0, 0, 1, 0, 2, 6, p + 512, None) == 0      # y210: even is enough
    torch.cuda.synchronize()


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


def _stream_all(vs, frames, device=False):
    got = []
    for f in frames:
        got += vs.push(_cuda(np.array(f)) if device else f)
        got += vs.pop_ready()
    got += vs.end()
    got = [(i, _numpy(f) if torch.is_tensor(f) else f) for i, f in got]
    assert [i for i, _ in got] == list(range(len(frames)))
    return np.stack([f for _, f in got])


def _both_containers(vs, frames, want):
    for device in (False, True):
        got = _stream_all(vs, frames, device)
        assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, got.shape, want.shape)
        assert np.array_equal(got, want), (device, int((got != want).sum()))
        vs.reset()                                                       # the packing survives


def test_yuyv_in_uyvy_out_equals_pack_of_the_planar_422_session(engines):
    planes = _planes(F, H, W, seed=81)
    with engines[1].open_stream(H, W, BATCH, pixel_format="i420", matrix="bt601", chroma="422", chroma_siting="center") as vs:
        planar = _stream_all(vs, [yuv.pack(*p, "i420", "422") for p in planes])
    want = np.stack([P.pack(yuv.planes(f, "i420", 4 * H, 4 * W, "422"), "uyvy422", 4 * H, 4 * W) for f in planar])
    with engines[0].open_stream(H, W, BATCH, pixel_format="nv12", matrix="bt601", chroma="422", chroma_siting="center", packing="yuyv422",
                                out_packing="uyvy422") as vs:
        assert (vs.packing, vs.out_packing) == ("yuyv422", "uyvy422")
        _both_containers(vs, [P.pack(p, "yuyv422", H, W) for p in planes], want)


def test_bgra_in_rgba_out_equals_pack_of_the_rgb24_session(engines):
    rgb = _rgb_frames(F, H, W, seed=82)
    with engines[1].open_stream(H, W, BATCH) as vs:
        sr = _stream_all(vs, list(rgb))
    want = np.stack([P.pack(f, "rgba", 4 * H, 4 * W) for f in sr])
    with engines[0].open_stream(H, W, BATCH, packing="bgra", out_packing="rgba") as vs:
        _both_containers(vs, [P.pack(f, "bgra", H, W) for f in rgb], want)
    with engines[0].open_stream(H, W, BATCH, pixel_format="nv12", chroma="422", packing="yuyv422", out_format="rgb24", out_packing="bgra") as vs:
        assert vs.out_packing == "bgra"                                  # a capture card in, a swap chain out: the issue's own line opens


def test_v210_in_y210_out_equals_pack_of_the_planar_10_bit_422_session(engines):
    planes = _planes(F, H, W, seed=83, levels=1024)
    with engines[1].open_stream(H, W, BATCH, pixel_format="i420", out_format="i010", in_depth=10, chroma="422") as vs:
        planar = _stream_all(vs, [depth10.pack10(*p, "i010", "422") for p in planes])
    want = np.stack([P.pack(depth10.planes10(f, "i010", 4 * H, 4 * W, "422"), "y210", 4 * H, 4 * W) for f in planar])
    with engines[0].open_stream(H, W, BATCH, pixel_format="i420", out_format="i010", in_depth=10, chroma="422", packing="v210",
                                out_packing="y210") as vs:
        _both_containers(vs, [P.pack(p, "v210", H, W) for p in planes], want)


def test_x2bgr10_in_x2rgb10_out_equals_pack_of_the_rgb10_session(engines):
    rgb = _rgb_frames(F, H, W, seed=84, levels=1024)
    with engines[1].open_stream(H, W, BATCH, in_depth=10, out_format="rgb10") as vs:
        sr = _stream_all(vs, list(rgb))
    want = np.stack([P.pack(f, "x2rgb10", 4 * H, 4 * W) for f in sr])
    with engines[0].open_stream(H, W, BATCH, in_depth=10, out_format="rgb10", packing="x2bgr10", out_packing="x2rgb10") as vs:
        _both_containers(vs, [P.pack(f, "x2bgr10", H, W) for f in rgb], want)


def test_an_output_size_with_a_packed_output_equals_from_rgb_of_the_resized_rgb(engines):
    rgb = _rgb_frames(F, H, W, seed=85)
    out_size = (45, 90)                                                  # v210: 90 = 15 groups, 240 bytes in rows of 256
    with engines[1].open_stream(H, W, BATCH, out_format="rgb10", out_size=out_size) as vs:
        sr = _stream_all(vs, list(rgb))
    want = np.stack([P.from_rgb(f, "v210", "bt709", False, "left") for f in sr])
    assert want.shape == (F, 45, 256)
    with engines[0].open_stream(H, W, BATCH, out_format="i010", out_chroma="422", out_size=out_size, out_packing="v210") as vs:
        _both_containers(vs, list(rgb), want)
    with pytest.raises(ValueError, match="multiple of 6"):               # refused before anything touches the engine
        engines[0].open_stream(H, W, BATCH, out_format="i010", out_chroma="422", out_size=(45, 92), out_packing="v210")


def test_planes_on_pitched_device_tensors_keep_their_padding(engines):
    planes = _planes(F, H, W, seed=86)
    frames = [P.pack(p, "yuyv422", H, W) for p in planes]
    oH, oW = 4 * H, 4 * W
    with engines[1].open_stream(H, W, BATCH, pixel_format="nv12", chroma="422", packing="yuyv422", out_packing="uyvy422") as vs:
        want = _stream_all(vs, frames)
    got = []
    with engines[0].open_stream(H, W, BATCH, pixel_format="nv12", chroma="422", packing="yuyv422", out_packing="uyvy422") as vs:
        def drain():
            while vs.ready():
                buf = torch.full((oH, 2 * oW + 48), 0xA5, dtype=torch.uint8, device="cuda")
                assert vs.pop_planes(*surface.views([buf], "nv12", oH, oW, "422", "uyvy422")) == len(got)
                host = buf.cpu().numpy()
                assert (host[:, 2 * oW:] == 0xA5).all()
                got.append(host[:, :2 * oW])

        for f in frames:
            buf = torch.from_numpy(surface.embed([f], [2 * W + 40], 0x3C)[0]).cuda()
            assert vs.push_planes(*surface.views([buf], "nv12", H, W, "422", "yuyv422")) == []
            assert (buf.cpu().numpy()[:, 2 * W:] == 0x3C).all()          # the surface itself is only read
            drain()
        vs._lib.pfnl_stream_end(vs._handle())
        drain()
    assert len(got) == F and all(np.array_equal(g, w_) for g, w_ in zip(got, want))


def test_setter_order_and_what_a_packing_holds_its_side_to(engines):
    frames = [P.pack(p, "yuyv422", H, W) for p in _planes(F, H, W, seed=87)]
    i420, rgb24 = _capi.PIXEL_FORMATS["i420"], _capi.PIXEL_FORMATS["rgb24"]
    yuyv, uyvy = _capi.PACKINGS["yuyv422"], _capi.PACKINGS["uyvy422"]
    with engines[1].open_stream(H, W, BATCH, pixel_format="i420", chroma="422", packing="yuyv422", out_packing="uyvy422") as vs:
        want = _stream_all(vs, frames)
    with engines[0].open_stream(H, W, BATCH, pixel_format="i420") as vs:
        lib, s = vs._lib, vs._s
        assert lib.pfnl_stream_packing(s, yuyv, uyvy) == -1 and b"chroma format" in lib.pfnl_last_error()     # before the chroma format: refused,
        assert lib.pfnl_stream_chroma_format(s, 1, 1) == 0
        assert lib.pfnl_stream_packing(s, yuyv, uyvy) == 0, lib.pfnl_last_error()                             # after it: accepted
        vs.chroma = vs.out_chroma = "422"                                                                     # (what the keywords would have noted)
        vs.packing, vs.out_packing = "yuyv422", "uyvy422"
        assert np.array_equal(_stream_all(vs, frames), want)
        vs.reset()
        for call in (lambda: lib.pfnl_stream_format(s, rgb24, rgb24, 1, 0), lambda: lib.pfnl_stream_chroma_format(s, 0, 0),
                     lambda: lib.pfnl_stream_input_depth(s, 10), lambda: lib.pfnl_stream_resize(s, 63, 95)):
            assert call() == -1                                                                               # a change under a packing: refused
        assert lib.pfnl_stream_format(s, rgb24, i420, 1, 0) == -1 and b"PFNL_PACK_NONE" in lib.pfnl_last_error()
        assert lib.pfnl_stream_packing(s, 10, 0) == -1 and lib.pfnl_stream_packing(s, 0, -1) == -1
        assert lib.pfnl_stream_packing(s, _capi.PACKINGS["bgra"], uyvy) == -1 and b"input" in lib.pfnl_last_error()
        assert lib.pfnl_stream_packing(s, yuyv, _capi.PACKINGS["y210"]) == -1 and b"output" in lib.pfnl_last_error()
        assert np.array_equal(_stream_all(vs, frames), want)                                                  # a refused call changes nothing
        vs.reset()
        vs.push(frames[0])
        assert lib.pfnl_stream_packing(s, 0, 0) == -2 and b"before the first frame" in lib.pfnl_last_error()  # PFNL_ERR_STATE
        vs.reset()
        assert lib.pfnl_stream_packing(s, 0, 0) == 0 and lib.pfnl_stream_chroma_format(s, 0, 0) == 0          # PFNL_PACK_NONE first, then the change
    for bad in ({"packing": "yuyv422"}, {"pixel_format": "nv12", "packing": "yuyv422"}, {"pixel_format": "nv12", "chroma": "422", "packing": "y210"},
                {"out_packing": "x2rgb10"}, {"packing": 4}, {"packing": "yuy2"}):
        with pytest.raises(ValueError):                                  # refused before anything touches the engine
            engines[0].open_stream(H, W, BATCH, **bad)


def test_a_session_without_a_packing_pops_the_explicit_paths_bytes(engines):
    """the planes of the layout, as always: gather_windows, forward, quantise_u8 on the same batches"""
    rgb = _rgb_frames(F, H, W, seed=88)
    dev = torch.from_numpy((rgb / 255.).astype(np.float32)).cuda()
    T = engines[1].geom.num_frames
    outs = []
    for first in range(0, F, BATCH):
        count = min(BATCH, F - first)
        outs.append(ops.quantise_u8(engines[1].forward(ops.gather_windows(dev, first, count, T)))[:, 0].cpu().numpy())
    with engines[0].open_stream(H, W, BATCH) as vs:
        assert (vs.packing, vs.out_packing) == (None, None)
        assert np.array_equal(_stream_all(vs, list(rgb)), np.concatenate(outs))
    with engines[0].open_stream(H, W, BATCH, packing="none", out_packing=None) as vs:
        assert np.array_equal(_stream_all(vs, list(rgb)), np.concatenate(outs))


# ---- the raw pipe ---------------------------------------------------------------------------------------------------------------------------
def test_rawvideo_on_a_yuyv422_stream_equals_the_session_driven_directly(engines):
    frames = [P.pack(p, "yuyv422", H, W) for p in _planes(F, H, W, seed=89)]
    out, log = io.BytesIO(), io.StringIO()
    reader = rawvideo.RawReader(io.BytesIO(b"".join(f.tobytes() for f in frames)), "yuyv422", H, W)
    assert rawvideo.run(reader, rawvideo.RawWriter(out), engines[0].open_stream, out_format="uyvy422", batch=BATCH, matrix="bt601", log=log) == F
    with engines[1].open_stream(H, W, BATCH, pixel_format="i420", out_format="i420", matrix="bt601", chroma="422", out_chroma="422",
                                packing="yuyv422", out_packing="uyvy422") as vs:
        want = _stream_all(vs, frames)
    assert out.getvalue() == want.tobytes() and "5 frames" in log.getvalue()
