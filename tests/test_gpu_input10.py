"""10-bit input on a real MI355X (include/pfnl_hip.h 10 BITS IN: pfnl_stream_input_depth and the pfnl_op_*_u10 input hooks): the decode of
P010 / I010, the gathers and the scene sum of the 16-bit ring, and the session built on them, against the host rule (pfnl_amd/depth10.py
to_rgb10 / values10 / dequantise10, pfnl_amd/scene.py luma_u10).  Everything is exact: samples with np.array_equal, fp32 windows bit for bit."""
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfnl_amd import model as M  # noqa: E402
from pfnl_amd import _capi, depth10, ops, scene, surface, synth, y4m, yuv  # noqa: E402
from pfnl_amd import upscale as up  # noqa: E402
from pfnl_amd.engine import PFNLEngine  # noqa: E402
from pfnl_amd.spec import PFNLGeometry  # noqa: E402

GEOM = PFNLGeometry(num_block=1)
T = GEOM.num_frames
H, W = 16, 24
PAIRS = [("bt601", False), ("bt601", True), ("bt709", False), ("bt709", True)]
# (2, 2), (2, 6), (6, 2): nothing but edges; (18, 34), (34, 66): single samples, W / 2 odd; (10, 36): W % 8 != 0; (16, 64): 16-byte words
SHAPES = [(2, 2), (2, 6), (6, 2), (18, 34), (34, 66), (10, 36), (16, 64)]


def _dev16(a):
    """a uint16 numpy array on the device as torch.uint16 (through int16: the copy kernels all know that type)"""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda().view(torch.uint16)


def _host16(t):
    assert t.dtype == torch.uint16
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _values(rng, shape):
    """random 10-bit values, every one of the 1024 present where they fit"""
    a = rng.integers(0, 1024, size=shape, dtype=np.uint16)
    flat = a.reshape(-1)
    if flat.size >= 1024:
        flat[rng.permutation(flat.size)[:1024]] = np.arange(1024, dtype=np.uint16)
        assert len(np.unique(flat)) == 1024
    return a


def _as_memory(rng, values, fmt):
    """10-bit values as a decoder's memory may hold them: P010 with random low six bits, I010 / RGB10 with a few samples above 1023 where
    the value is 1023 - what values10 takes back to `values`"""
    if fmt == "p010":
        return ((values << 6) | rng.integers(0, 64, values.shape).astype(np.uint16)).astype(np.uint16)
    out = values.copy()
    top = np.flatnonzero(out.reshape(-1) == 1023)
    if top.size:
        pick = top[::2]
        out.reshape(-1)[pick] = rng.integers(1024, 65536, pick.size).astype(np.uint16)
    return out


def _yuv10_frames(n, h, w, fmt, seed):
    """n packed frames [n, h*3/2, w] as memory holds them; the last one 0 / 1023 in blocks, so that both clips fire"""
    rng = np.random.default_rng(seed)
    vals = [_values(rng, (h * 3 // 2, w)) for _ in range(n)]
    small = rng.integers(0, 2, size=((h * 3 // 2 + 1) // 2, (w + 1) // 2)).astype(np.uint16) * 1023
    vals[-1] = np.repeat(np.repeat(small, 2, 0), 2, 1)[:h * 3 // 2, :w]
    frames = np.stack([_as_memory(rng, v, fmt) for v in vals])
    assert np.array_equal(depth10.values10(frames, fmt), np.stack(vals))
    return frames


# ---- 1. the decode op ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", SHAPES)
@pytest.mark.parametrize("fmt", depth10.FORMATS)
def test_decode_equals_to_rgb10(fmt, h, w):
    for n in (1, 3):
        frames = _yuv10_frames(n, h, w, fmt, seed=h * w + n)
        if fmt == "p010":
            assert (frames & 63).any()
        elif frames.size >= 1024:
            assert (frames > 1023).any()
        d = _dev16(frames)
        assert d.data_ptr() % 16 == 0
        for matrix, full in PAIRS:
            for siting in yuv.SITINGS:
                want = np.stack([depth10.to_rgb10(f, fmt, h, w, matrix, full, siting) for f in frames])
                got = _host16(ops.yuv420_to_rgb10(d, fmt, h, w, matrix, full, siting=siting))
                assert got.shape == (n, h, w, 3) and np.array_equal(got, want), (n, matrix, full, siting, int((got != want).sum()))
                if h * w >= 64:
                    assert (want[-1] == 0).any() and (want[-1] == 1023).any()  # both clips fire on the frame of extremes


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


# ---- 2. one sample off: the narrow form -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(16, 64), (10, 36)])
@pytest.mark.parametrize("fmt", depth10.FORMATS)
def test_decode_at_a_pointer_one_sample_off(fmt, h, w):
    frames = _yuv10_frames(2, h, w, fmt, seed=7)
    for siting in yuv.SITINGS:
        want = np.stack([depth10.to_rgb10(f, fmt, h, w, "bt709", False, siting) for f in frames])
        got, intact = _guarded(lambda s, o: ops.yuv420_to_rgb10(s, fmt, h, w, "bt709", False, out=o, siting=siting), frames, want.size, 1)
        assert intact and np.array_equal(got.reshape(want.shape), want), siting


# ---- 3. pitched planes ------------------------------------------------------------------------------------------------------------------------
def _device_views(frame, fmt, h, w, extra):
    planes = surface.split(frame, fmt, h, w)
    bufs = surface.embed(planes, [p.shape[1] * 2 + extra for p in planes], fill=0xA5)
    return surface.views([torch.from_numpy(b).cuda() for b in bufs], fmt, h, w)


@pytest.mark.parametrize("fmt", depth10.FORMATS)
def test_decode_of_pitched_planes(fmt):
    for (h, w), extra in (((16, 64), 64), ((16, 64), 6), ((10, 36), 6), ((18, 34), 64)):
        frame = _yuv10_frames(1, h, w, fmt, seed=h + extra)[0]
        for siting in yuv.SITINGS:
            want = depth10.to_rgb10(frame, fmt, h, w, "bt601", False, siting)
            got = _host16(ops.yuv420_to_rgb10_surface(_device_views(frame, fmt, h, w, extra), fmt, h, w, "bt601", False, siting=siting))
            assert np.array_equal(got, want), (h, w, extra, siting)
    # a window inside a larger surface: the planes start at the window's first sample and keep the surface's pitch
    bh, bw, y0, x0, h, w = 24, 48, 4, 8, 16, 32
    big = _yuv10_frames(1, bh, bw, fmt, seed=99)[0]
    views = _device_views(big, fmt, bh, bw, 64)
    if fmt == "p010":
        win = (views[0][y0:y0 + h, x0:x0 + w], views[1][y0 // 2:(y0 + h) // 2, x0:x0 + w])
    else:
        win = (views[0][y0:y0 + h, x0:x0 + w],) + tuple(v[y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2] for v in views[1:])
    host = surface.split(big, fmt, bh, bw)
    if fmt == "p010":
        cut = [host[0][y0:y0 + h, x0:x0 + w], host[1][y0 // 2:(y0 + h) // 2, x0:x0 + w]]
    else:
        cut = [host[0][y0:y0 + h, x0:x0 + w]] + [p[y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2] for p in host[1:]]
    packed = np.concatenate([c.reshape(-1) for c in cut])
    for siting in yuv.SITINGS:
        want = depth10.to_rgb10(packed, fmt, h, w, "bt709", True, siting)
        assert np.array_equal(_host16(ops.yuv420_to_rgb10_surface(win, fmt, h, w, "bt709", True, siting=siting)), want), siting


# ---- 4. the gather --------------------------------------------------------------------------------------------------------------------------
def _ring_samples(rng, shape):
    a = rng.integers(0, 1024, size=shape).astype(np.uint16)
    over = rng.random(shape) < 0.05
    a[over] = rng.integers(1024, 65536, int(over.sum())).astype(np.uint16)     # above 1023: the table's last entry
    a.reshape(-1)[0] = 65535                                                    # (one at least, whatever the size)
    return a


# (last, first, count): windows that clamp at frame 0 and at `last`, and rings that wrap; at most `cap` frames named
GATHERS = {5: [(2, 0, 3), (9, 6, 1), (9, 8, 2)], 7: [(3, 0, 2), (8, 8, 1), (11, 10, 2)]}


@pytest.mark.parametrize("h,w", [(2, 2), (4, 8), (6, 10)])       # 24 bytes a frame: 4-byte words; 192: 16-byte words; 360: 4-byte words
@pytest.mark.parametrize("Tn", [5, 7])
def test_gather_windows_u10_equals_dequantise10(Tn, h, w):
    cap, F = 5, 13
    rng = np.random.default_rng(Tn * h * w)
    seq = _ring_samples(rng, (F, h, w, 3))
    assert (seq > 1023).any()
    for last, first, count in GATHERS[Tn]:
        lo, hi = max(0, first - Tn // 2), min(last, first + count - 1 + Tn // 2)
        assert hi - lo + 1 <= cap
        ring = _ring_samples(rng, (cap, h, w, 3))                               # slots the windows do not name hold other samples
        for f in range(lo, hi + 1):
            ring[f % cap] = seq[f]
        idx = np.clip(np.arange(first, first + count)[:, None] + np.arange(-(Tn // 2), Tn // 2 + 1)[None, :], 0, last)
        want = depth10.dequantise10(seq)[idx]
        got = ops.gather_windows_u10(_dev16(ring), last, first, count, Tn).cpu().numpy()
        assert got.dtype == np.float32 and got.shape == want.shape == (count, Tn, h, w, 3)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (last, first, count)   # bit for bit


# ---- 5. the scene-aware gather ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(4, 8), (6, 10)])
def test_gather_windows_u10_scenes_equals_the_host_rule(h, w):
    F, cap, Tn = 14, 9, 5
    rng = np.random.default_rng(h + w)
    seq = _ring_samples(rng, (F, h, w, 3))
    sf = np.zeros((F,), np.int64)
    for f in range(1, F):
        sf[f] = f if f in (5, 8) else sf[f - 1]                                 # three scenes: 0 .. 4, 5 .. 7, 8 ..
    for last, first, count in [(11, 3, 5), (9, 7, 3), (13, 10, 2)]:
        lo, hi = max(0, first - Tn // 2), min(last, first + count - 1 + Tn // 2)
        assert hi - lo + 1 <= cap
        ring = _ring_samples(rng, (cap, h, w, 3))
        table = np.full((cap,), 12345, np.int64)
        for f in range(lo, hi + 1):
            ring[f % cap] = seq[f]
            table[f % cap] = sf[f]
        idx = scene.scene_windows_index(sf, Tn, last)[first:first + count]
        want = depth10.dequantise10(seq)[idx]
        got = ops.gather_windows_u10_scenes(_dev16(ring), torch.from_numpy(table).cuda(), last, first, count, Tn).cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (last, first, count)
    one = np.zeros((cap,), np.int64)                                            # one scene: the plain windows
    ring = _dev16(seq[:cap])
    a = ops.gather_windows_u10_scenes(ring, torch.from_numpy(one).cuda(), 6, 2, 3, Tn).cpu().numpy()
    b = ops.gather_windows_u10(ring, 6, 2, 3, Tn).cpu().numpy()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- 6. the scene sum -------------------------------------------------------------------------------------------------------------------------
# 1 pixel: the tail alone; 15: 12-byte groups and a tail; 32 (192 bytes): 48-byte groups; 384: more than one lane's worth of groups
@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (4, 8), (16, 24)])
def test_scene_sad_u10_is_exact(h, w):
    rng = np.random.default_rng(h * w)
    a, b = _ring_samples(rng, (2, h, w, 3))
    zeros, ones = np.zeros((h, w, 3), np.uint16), np.full((h, w, 3), 1023, np.uint16)
    far = np.full((h, w, 3), 65535, np.uint16)                                  # counts as 1023
    for x, y in [(a, b), (b, a), (a, a), (zeros, ones), (ones, zeros), (zeros, far), (ones, far)]:
        want = scene.frame_sad10(x, y)
        dx, dy = _dev16(x), _dev16(y)
        assert ops.scene_sad_u10(dx, dy) == want
        assert ops.scene_sad_u10(dx, dy) == want                                # back to back: every launch leaves its scratch zeroed
    assert scene.frame_sad10(zeros, ones) == 220 * h * w == scene.frame_sad10(zeros, far) and scene.frame_sad10(ones, far) == 0
    n = h * w * 3                                                               # frames one sample behind an aligned address
    buf = _dev16(np.concatenate([[0], a.ravel(), [0, 0], b.ravel()]).astype(np.uint16))
    x, y = buf[1:1 + n].view(h, w, 3), buf[n + 3:2 * n + 3].view(h, w, 3)
    assert x.data_ptr() % 4 == 2 and ops.scene_sad_u10(x, y) == scene.frame_sad10(a, b)


# ---- the session ------------------------------------------------------------------------------------------------------------------------------
def _engine_with(w, precision="fp32"):
    e = PFNLEngine(GEOM, device=0)
    e.load_weights(w)
    if precision != "fp32":
        e.set_option("precision", precision)
    return e


@pytest.fixture(scope="module")
def engines():
    w = synth.synthetic_weights(GEOM, seed=0)
    pair = _engine_with(w), _engine_with(w)
    yield pair
    for e in pair:
        e.close()


def _to_device(f):
    return _dev16(f) if f.dtype == np.uint16 else torch.from_numpy(f).cuda()


def _to_host(f):
    if not torch.is_tensor(f):
        return f
    return _host16(f) if f.dtype == torch.uint16 else f.cpu().numpy()


def _stream_all(vs, frames, device=False):
    """push one frame at a time, pop after every push, then end: the delivered frames in order, as one numpy array"""
    got = []
    for f in frames:
        got += vs.push(_to_device(f) if device else f)
        got += vs.pop_ready()
    got += vs.end()
    assert [i for i, _ in got] == list(range(len(frames)))
    assert all((torch.is_tensor(f) and f.is_cuda) == device for _, f in got)
    return np.stack([_to_host(f) for _, f in got])


def _explicit(eng, frames_u10, batch, quantise):
    """the session's batches through the single ops on `eng`: quantise(forward(dequantise10(frames)[the windows' index]))"""
    win = M.sliding_windows(depth10.dequantise10(frames_u10), T)
    outs = []
    for first in range(0, len(win), batch):
        x = torch.from_numpy(np.ascontiguousarray(win[first:first + batch])).cuda()
        outs.append(_to_host(quantise(eng.forward(x))[:, 0]))
    return np.concatenate(outs)


def _rgb10_sequence(F, seed, h=H, w=W):
    rng = np.random.default_rng(seed)
    return np.stack([_as_memory(rng, _values(rng, (h, w, 3)), "rgb10") for _ in range(F)])


# ---- 7. RGB10-layout in -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,batch,precision", [(9, 4, "fp32"), (5, 3, "fp32"), (2, 5, "fp32"), (9, 4, "bf16")])
def test_session_rgb10_in_equals_the_explicit_path(F, batch, precision):
    w = synth.synthetic_weights(GEOM, seed=0)
    eng, eng2 = _engine_with(w, precision), _engine_with(w, precision)
    lr = _rgb10_sequence(F, seed=10 * F + batch)
    assert (lr > 1023).any()
    for fmt, quantise in (("rgb24", ops.quantise_u8), ("rgb10", ops.quantise_u10)):
        want = _explicit(eng2, lr, batch, quantise)
        assert want.shape == (F, 4 * H, 4 * W, 3) and len(np.unique(want)) > 64  # (frames with content)
        with eng.open_stream(H, W, batch, out_format=fmt, in_depth=10) as vs:
            assert (vs.pixel_format, vs.out_format, vs.in_depth) == ("rgb24", fmt, 10)
            for device in (False, True):
                got = _stream_all(vs, list(lr), device)
                assert got.dtype == want.dtype and np.array_equal(got, want), (fmt, device, int((got != want).sum()))
                vs.reset()                                                      # the depth and the format survive
    eng.close()
    eng2.close()


# ---- 8. P010 / I010 in ------------------------------------------------------------------------------------------------------------------------
CASES_420 = [("nv12", "p010", "i010", "bt709", False, {}), ("i420", "i010", "i420", "bt601", False, {}), ("nv12", "p010", "rgb24", "bt601", True, {}),
             ("i420", "i010", "i010", "bt709", False, {"chroma_siting": "center", "out_size": (36, 54)})]


@pytest.mark.parametrize("layout,fmt,out_fmt,matrix,full,extra", CASES_420)
def test_session_yuv10_in_equals_the_rgb_session_fed_to_rgb10(engines, layout, fmt, out_fmt, matrix, full, extra):
    F, batch = 7, 3
    frames = _yuv10_frames(F, H, W, fmt, seed=len(out_fmt) + F)
    rgb = np.stack([depth10.to_rgb10(f, fmt, H, W, matrix, full, extra.get("chroma_siting", "left")) for f in frames])
    kw = dict(out_format=out_fmt, matrix=matrix, full_range=full, in_depth=10, out_size=extra.get("out_size"))
    with engines[1].open_stream(H, W, batch, out_chroma_siting=extra.get("chroma_siting", "left"), **kw) as vs:
        want = _stream_all(vs, list(rgb))
    assert len(np.unique(want)) > 16
    with engines[0].open_stream(H, W, batch, pixel_format=layout, chroma_siting=extra.get("chroma_siting", "left"), **kw) as vs:
        for device in (False, True):
            got = _stream_all(vs, [f.reshape(-1) for f in frames] if not device else list(frames), device)
            assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want), (device, int((got != want).sum()))
            vs.reset()


# ---- 9. planes with a pitch equal the packed push -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,fmt", [("nv12", "p010"), ("i420", "i010"), ("rgb24", "rgb10")])
def test_push_planes_equals_push(engines, layout, fmt):
    F, batch = 5, 2
    frames = _rgb10_sequence(F, 5) if fmt == "rgb10" else _yuv10_frames(F, H, W, fmt, seed=5)
    with engines[0].open_stream(H, W, batch, pixel_format=layout, out_format="rgb24", in_depth=10) as vs:
        want = _stream_all(vs, list(frames))
        for device in (False, True):
            vs.reset()
            got = []
            for k, f in enumerate(frames):
                planes = surface.split(f, fmt, H, W)
                bufs = surface.embed(planes, [p.shape[1] * 2 + (64 if k % 2 else 6) for p in planes], fill=0x5A)
                views = surface.views([torch.from_numpy(b).cuda() for b in bufs] if device else bufs, fmt, H, W)
                got += vs.push_planes(*views)
                got += vs.pop_ready()
            got += vs.end()
            assert [i for i, _ in got] == list(range(F))
            assert np.array_equal(np.stack([_to_host(f) for _, f in got]), want), device


# ---- 10. scenes -------------------------------------------------------------------------------------------------------------------------------
def test_scenes_at_depth_10(engines):
    batch, thr = 3, 20.0
    rng = np.random.default_rng(77)
    frames = []
    for n in (5, 4, 6):                                                         # two hard cuts: frames 5 and 9
        base = rng.integers(0, 1024, size=(H, W, 3))
        frames += [np.clip(base + rng.integers(-8, 9, size=(H, W, 3)), 0, 1023).astype(np.uint16) for _ in range(n)]
    frames[11] = frames[12] = frames[10].copy()                                 # a flat stretch: sums of zero
    sads = scene.frame_sads10(frames)
    sf = scene.scene_first(frames, thr, depth=10)
    assert sf.tolist() == [0] * 5 + [5] * 4 + [9] * 6 and sads[11] == sads[12] == 0 < sads[13]
    for device in (False, True):
        with engines[0].open_stream(H, W, batch, scene_cut=thr, in_depth=10) as vs:
            got, infos = [], []
            for f in frames + [None]:
                if f is None:
                    _capi.check(vs._lib.pfnl_stream_end(vs._s))
                else:
                    assert vs.push(_to_device(f) if device else f) == []
                while True:
                    item = vs.pop()
                    if item is None:
                        break
                    got.append(_to_host(item[1]))
                    infos.append(vs.last_info)
            assert vs.cuts == [5, 9] and infos == [(int(a), int(b)) for a, b in zip(sf, sads)]
        alone = []
        for a, b in ((0, 5), (5, 9), (9, 15)):
            with engines[1].open_stream(H, W, batch, in_depth=10) as vs:
                alone.append(_stream_all(vs, frames[a:b]))
        assert np.array_equal(np.stack(got), np.concatenate(alone)), device


# ---- 11. the range fence ----------------------------------------------------------------------------------------------------------------------
def test_recomputed_batches_are_regathered_from_the_16_bit_ring():
    """The setup of tests/test_gpu_yuv.py test_recomputed_batches_leave_in_the_output_format (conv0 x 4e5 leaves binary16's range,
    convmerge2 x 1e-6 brings the result back onto the scale of the samples): every batch is delivered from the strict kernels' result."""
    h, w_, batch = 12, 20, 3
    lr = _rgb10_sequence(7, 21, h, w_)
    w = synth.synthetic_weights(GEOM, seed=1)
    w["nlvsr/conv0/kernel"] = (w["nlvsr/conv0/kernel"] * 4e5).astype(np.float32)
    w["nlvsr/convmerge2/kernel"] = (w["nlvsr/convmerge2/kernel"] * 1e-6).astype(np.float32)
    eng, strict = _engine_with(w), _engine_with(w)
    with eng.open_stream(h, w_, batch, out_format="rgb10", in_depth=10) as vs:
        got = _stream_all(vs, list(lr))
        assert eng.get_option("strict_fp32") == "off"                           # end + the last pop have put it back
    strict.set_option("strict_fp32", "on")
    sr = strict.forward(np.ascontiguousarray(M.sliding_windows(depth10.dequantise10(lr), T)))
    assert np.isfinite(sr).all()
    want = depth10.quantise10(sr[:, 0])
    assert np.array_equal(got, want) and len(np.unique(want)) > 16
    assert eng.range_flagged() is False
    eng.close()
    strict.close()


# ---- 12. state and validation -------------------------------------------------------------------------------------------------------------------
def test_state_and_validation(engines):
    eng = engines[0]
    lib, batch = eng._lib, 2
    lr10 = list(_rgb10_sequence(6, 61))
    lr8 = list(np.random.default_rng(62).integers(0, 256, (6, H, W, 3), np.uint8))
    with eng.open_stream(H, W, batch) as vs:
        plain = _stream_all(vs, lr8)
        vs.reset()
        assert lib.pfnl_stream_input_depth(vs._s, 8) == 0                       # 8: the session it always was
        assert np.array_equal(_stream_all(vs, lr8), plain)
    with eng.open_stream(H, W, batch, in_depth=10) as vs:
        first = _stream_all(vs, lr10)
        vs.reset()
        for bits in (12, 16, 0, 9):
            assert lib.pfnl_stream_input_depth(vs._s, bits) == -1 and b"8 or 10" in lib.pfnl_last_error()
        for in_fmt in (3, 4, 5):                                                # the 10-bit names stay refused as in_fmt
            assert lib.pfnl_stream_format(vs._s, in_fmt, 0, 1, 0) == -1 and b"10-bit input" in lib.pfnl_last_error()
        assert lib.pfnl_stream_format(vs._s, 1, 3, 1, 0) == -1 and b"RGB10" in lib.pfnl_last_error()
        vs.push(lr10[0])
        assert lib.pfnl_stream_input_depth(vs._s, 8) == -2 and b"before the first frame" in lib.pfnl_last_error()
        assert lib.pfnl_stream_input_depth(vs._s, 12) == -1                     # (a bad depth is a bad depth at any time)
        got = vs.pop_ready()                                                    # ... and nothing changed: the sequence carries on
        for f in lr10[1:]:
            got += vs.push(f)
            got += vs.pop_ready()
        got += vs.end()
        assert np.array_equal(np.stack([f for _, f in got]), first)
        vs.reset()                                                              # the depth survives reset and a later pfnl_stream_format
        assert lib.pfnl_stream_format(vs._s, 0, 3, 1, 0) == 0
        vs.out_format = "rgb10"                                                 # (the raw call went past the Python object)
        wide = _stream_all(vs, lr10)
        # the same fp32 value rounded to 1023 levels and to 255: |v10 / 1023 - v8 / 255| <= 0.5 / 1023 + 0.5 / 255, over 2 * 1023 * 255
        assert wide.dtype == np.uint16 and int(np.abs(2 * (255 * wide.astype(np.int64) - 1023 * first.astype(np.int64))).max()) <= 255 + 1023
        vs.reset()
        assert lib.pfnl_stream_format(vs._s, 0, 0, 1, 0) == 0 and lib.pfnl_stream_input_depth(vs._s, 8) == 0   # back to 8 bits on an open session
        vs.out_format, vs.in_depth = "rgb24", 8
        assert np.array_equal(_stream_all(vs, lr8), plain)
        vs.reset()
        assert lib.pfnl_stream_input_depth(vs._s, 10) == 0                      # and to 10 again
        vs.in_depth = 10
        assert np.array_equal(_stream_all(vs, lr10), first)
    for bad in (12, None):
        with pytest.raises(ValueError, match="in_depth"):
            eng.open_stream(H, W, batch, in_depth=bad)
    with eng.open_stream(H, W, batch, in_depth=10) as vs:                       # (nothing was left open by the refusals)
        with pytest.raises(ValueError, match="uint16"):
            vs.push(lr8[0])
        with pytest.raises(ValueError, match="uint16"):
            vs.push(torch.from_numpy(lr8[0]).cuda())
        assert np.array_equal(_stream_all(vs, lr10), first)


# ---- 13. Y4M end to end -----------------------------------------------------------------------------------------------------------------------
def test_upscale_of_a_10_bit_stream_equals_the_session_driven_directly(engines):
    F, batch = 6, 2
    frames = list(_yuv10_frames(F, H, W, "i010", seed=13))
    frames = [np.minimum(f, 1023).astype(np.uint16) for f in frames]            # (a file holds the values themselves)
    data = b"YUV4MPEG2 W24 H16 F25:1 Ip A1:1 C420p10 XYSCSS=420P10\n" + b"".join(b"FRAME\n" + f.astype("<u2").tobytes() for f in frames)
    out, log = io.BytesIO(), io.StringIO()
    n = up.upscale(y4m.Y4MReader(io.BytesIO(data), depths=(8, 10)), y4m.Y4MWriter(out), engines[0].open_stream, batch=batch, out_format="i010", log=log)
    assert n == F
    with engines[1].open_stream(H, W, batch, pixel_format="i420", out_format="i010", matrix="bt601", full_range=False, chroma_siting="left",
                                in_depth=10) as vs:
        want = _stream_all(vs, frames)
    head, body = out.getvalue().split(b"\n", 1)
    assert head == b"YUV4MPEG2 W96 H64 F25:1 Ip A1:1 C420p10 XYSCSS=420P10"
    assert body == b"".join(b"FRAME\n" + f.astype("<u2").tobytes() for f in want) and len(np.unique(want)) > 16
