"""The content box on a real MI355X (include/pfnl_hip.h BARS; pfnl_amd/csrc/bars.hip): the op hooks at both depths in their 16-byte, 4-byte
and single-sample forms against pfnl_amd/bars.py - boxes, row sums and column sums exact -, sessions with ``bars=`` against the rule applied
to the frames their ring holds, and ``upscale --crop`` against the stream cropped on the host beforehand.  No tolerance anywhere."""
import ctypes as C
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import bars_gen as G  # noqa: E402
from pfnl_amd import _capi, bars, deinterlace, ops, synth, y4m, yuv  # noqa: E402
from pfnl_amd import telecine as TC  # noqa: E402
from pfnl_amd import upscale as up  # noqa: E402
from pfnl_amd.engine import PFNLEngine  # noqa: E402
from pfnl_amd.spec import PFNLGeometry  # noqa: E402

# (2, 2): one strip, one lane; (6, 10): single pixels at 8 bits (2-pixel words at 10); (8, 20): 4-pixel words at 8 bits; (16, 64): 16-byte
# words at both depths, two strips; (33, 50): five strips, the last one row long; (1030, 16): 129 strips draw tickets; (4, 4112): 257 groups
# of 16 pixels - a row longer than one pass of a workgroup's 256 lanes
SHAPES = [(2, 2), (6, 10), (8, 20), (16, 64), (33, 50), (1030, 16), (4, 4112)]
LIMIT = 8


def _cuda(a):
    a = np.ascontiguousarray(a)                                          # (torch copies int16, not uint16)
    return torch.from_numpy(a).cuda() if a.dtype == np.uint8 else torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)


def _numpy(t):
    if t.dtype == torch.uint16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    if t.dtype == torch.uint32:
        return t.view(torch.int32).cpu().numpy().view(np.uint32)
    return t.cpu().numpy()


def _at_offset(a, off):
    """``a`` in a device buffer, ``off`` bytes behind a 256-byte boundary"""
    nbytes = a.size * a.itemsize
    buf = torch.zeros((off + nbytes + 64,), dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    raw = buf[off:off + nbytes]
    raw.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8)).cuda())
    return buf, (raw if a.dtype == np.uint8 else raw.view(torch.uint16)).view(a.shape)


_FRAMES = {}


def _frames(H, W, maxv):
    """(frames, their boxes, row sums and column sums by the rule), made once per shape and depth"""
    key = (H, W, maxv)
    if key not in _FRAMES:
        depth = 10 if maxv == 1023 else 8
        fs = list(G.cases(H, W, maxv).values()) + [G.at_threshold(H, W, LIMIT, maxv), G.at_threshold(H, W, LIMIT, maxv, over=True)]
        sums = [bars.line_sums(f, depth) for f in fs]
        _FRAMES[key] = (fs, [bars.box(r, c, H, W, LIMIT) for r, c in sums], [r for r, _ in sums], [c for _, c in sums])
    return _FRAMES[key]


def _check(got, want_boxes, want_rows, want_cols, what):
    box, rows, cols = got
    assert [tuple(b) for b in box.cpu().tolist()] == list(want_boxes), what
    assert np.array_equal(_numpy(rows).astype(np.int64), np.stack(want_rows)), what
    assert np.array_equal(_numpy(cols).astype(np.int64), np.stack(want_cols)), what


# ---- the ops --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("maxv", [255, 1023])
@pytest.mark.parametrize("H,W", SHAPES)
def test_the_op_is_the_rule(H, W, maxv):
    fs, boxes, rows, cols = _frames(H, W, maxv)
    assert boxes[-2] == (0, 0, 0, 0) and boxes[-1] == (H // 2, W // 3, 1, 1)   # sums at the threshold are no picture, one above is
    assert (0, 0, 0, 0) in boxes[:-2] and (0, 0, H, W) in boxes
    dev = _cuda(np.stack(fs))
    for _ in range(2):                                                   # the same call twice: the same answer
        _check(ops.content_box(dev, LIMIT, sums=True), boxes, rows, cols, (H, W, maxv, "all"))
    _check(ops.content_box(dev[:3], LIMIT, sums=True), boxes[:3], rows[:3], cols[:3], (H, W, maxv, "n = 3"))
    for k in (0, len(fs) - 1):                                           # n = 1, as a [H, W, 3] frame and without the sums
        _check(ops.content_box(dev[k], LIMIT, sums=True), boxes[k:k + 1], rows[k:k + 1], cols[k:k + 1], (H, W, maxv, "n = 1", k))
        assert tuple(ops.content_box(dev[k], LIMIT).cpu().tolist()[0]) == boxes[k]
    for limit in (0, 100, 219):                                          # other limits, the largest included
        want = [bars.box(r, c, H, W, limit) for r, c in zip(rows, cols)]
        assert [tuple(b) for b in ops.content_box(dev, limit).cpu().tolist()] == want, (H, W, maxv, limit)


@pytest.mark.parametrize("maxv", [255, 1023])
@pytest.mark.parametrize("H,W", SHAPES)
def test_offset_base_pointers_take_the_narrow_forms(H, W, maxv):
    """one sample off a 256-byte boundary: single samples whatever the width; four bytes off it: 4-byte words where the rows allow"""
    fs, boxes, rows, cols = _frames(H, W, maxv)
    pick = [0, 4, 7, len(fs) - 1]                                        # middle, right, noisy, one above the threshold
    host = np.stack([fs[k] for k in pick])
    for off in (host.itemsize, 4):
        buf, view = _at_offset(host, off)
        assert view.data_ptr() % 16 == off
        _check(ops.content_box(view, LIMIT, sums=True), [boxes[k] for k in pick], [rows[k] for k in pick], [cols[k] for k in pick], (H, W, maxv, off))
        assert np.array_equal(_numpy(view), host)                        # the frames are only read


def test_a_smaller_frame_after_a_larger_one():
    """what a launch leaves behind does not reach the next one on the same stream"""
    for maxv in (255, 1023):
        big, small = _frames(33, 50, maxv), _frames(6, 10, maxv)
        for fs, boxes, rows, cols in (big, small, big, small):
            _check(ops.content_box(_cuda(np.stack(fs)), LIMIT, sums=True), boxes, rows, cols, maxv)


def test_the_hooks_refuse_before_any_launch():
    lib = _capi.load_library()
    buf = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    ok = [p, 1, 4, 8, LIMIT, p + 4096, p + 4352, p + 4608, None]
    for hook in (lib.pfnl_op_content_box_u8, lib.pfnl_op_content_box_u10):
        assert hook(*ok) == 0
        for at, value in ((0, None), (5, None), (1, 0), (2, 0), (2, 16385), (3, 0), (3, 16385), (4, -1), (4, 220), (5, p + 4098), (6, p + 4354)):
            bad = list(ok)
            bad[at] = value
            assert hook(*bad) == -1, (at, value)
    bad = list(ok)
    bad[0] = p + 1
    assert lib.pfnl_op_content_box_u10(*bad) == -1 and lib.pfnl_op_content_box_u8(*bad) == 0
    with pytest.raises(ValueError):
        ops.content_box(buf[:96].view(4, 8, 3), limit=220)
    with pytest.raises(TypeError):
        ops.content_box(buf[:96].view(4, 8, 3).cpu())
    torch.cuda.synchronize()


# ---- the session ----------------------------------------------------------------------------------------------------------------------------
H, W, BATCH = 16, 24, 2


@pytest.fixture(scope="module")
def engine():
    geom = PFNLGeometry(num_block=1)
    e = PFNLEngine(geom, device=0)
    e.load_weights(synth.synthetic_weights(geom, seed=0))
    yield e
    e.close()


def _letterboxed(n, maxv=255):
    """n RGB frames of H x W whose picture moves and grows: no two boxes alike, the first frame black"""
    out = []
    for k in range(n):
        box = (4, 2 * (k % 3), 8, W - 4 * (k % 3)) if k % 2 else (2 + 2 * (k % 3), 0, 8, W - 2)
        out.append(G.boxed(H, W, box, maxv, seed=k, noise=3))
    out[0] = np.zeros_like(out[0])
    return out


def _drive(vs, frames, how="host"):
    """[(index, frame, box, running union)] of everything the session delivers"""
    seen, note = [], vs._note_info

    def noted(s, index):
        note(s, index)
        seen.append((vs.last_info["box"], vs.content_box) if vs.bars is not None else (None, None))

    vs._note_info = noted
    got = []
    for i, f in enumerate(frames):
        device = how == "device" or (how == "alt" and i % 2 == 1)
        got += vs.push(_cuda(np.array(f)) if device else f)
    got += vs.end()
    vs._note_info = note
    assert [i for i, _ in got] == list(range(len(got))) and len(seen) == len(got)
    return [(_numpy(f) if torch.is_tensor(f) else f, *seen[i]) for i, f in got]


def _check_session(engine, pushed, ring, depth, **kw):
    want = [bars.frame_box(f, LIMIT, depth) for f in ring]
    assert len(set(want)) > 2                                            # (the boxes differ from frame to frame)
    with engine.open_stream(H, W, BATCH, **kw) as vs:
        plain = [f for f, _, _ in _drive(vs, pushed, "alt")]
    assert len(plain) == len(ring)
    with engine.open_stream(H, W, BATCH, bars=LIMIT, **kw) as vs:
        assert vs.content_box is None
        for how in ("host", "alt", "device"):                            # across reset: the setting survives, the union starts again
            got = _drive(vs, pushed, how)
            assert [b for _, b, _ in got] == want, how
            assert [u for _, _, u in got] == [bars.union(want[:k + 1]) for k in range(len(want))], how
            assert vs.last_info[:2] == tuple(vs.last_info) and len(vs.last_info) == 2   # (scene_first, sad), as it always was
            for (a, _, _), b in zip(got, plain):                         # the SR bytes are those of the session without bars
                assert np.array_equal(a, b)
            vs.reset()
            assert vs.content_box is None and vs.last_info is None


def test_rgb_sessions_report_the_pushed_frames(engine):
    frames = _letterboxed(7)
    _check_session(engine, frames, frames, 8)
    frames10 = _letterboxed(7, 1023)
    _check_session(engine, frames10, frames10, 10, in_depth=10, out_format="rgb10")


def test_an_nv12_session_reports_the_decoded_frames(engine):
    pushed = [yuv.from_rgb(f, "nv12") for f in _letterboxed(7)]
    _check_session(engine, pushed, [yuv.to_rgb(f, "nv12", H, W) for f in pushed], 8, pixel_format="nv12", out_format="rgb24")


def test_an_interlaced_session_reports_the_deinterlaced_frames(engine):
    woven = _letterboxed(5)
    _check_session(engine, woven, deinterlace.frames(woven, "tff", "field"), 8, interlaced="field")


def test_a_telecine_session_reports_the_film_frames(engine):
    film = _letterboxed(8)
    pushed = TC.pulldown(film, 1, "tff")
    ring = TC.frames(pushed, "decimate", "tff")
    assert len(ring) == 8
    _check_session(engine, pushed, ring, 8, telecine="decimate")


def test_scenes_and_bars_travel_together(engine):
    frames = _letterboxed(7)
    with engine.open_stream(H, W, BATCH, scene_cut=10.0) as vs:
        want = [f for f, _, _ in _drive(vs, frames)]
        cuts = list(vs.cuts)
    with engine.open_stream(H, W, BATCH, scene_cut=10.0, bars=LIMIT) as vs:
        got = _drive(vs, frames, "alt")
        assert vs.cuts == cuts and [b for _, b, _ in got] == [bars.frame_box(f, LIMIT) for f in frames]
        assert vs.last_info["scene_first"] == vs.last_info[0] and vs.last_info["sad"] == vs.last_info[1]
        for (a, _, _), b in zip(got, want):
            assert np.array_equal(a, b)


def test_the_setting_and_its_refusals(engine):
    for bad in (-1, 220, 8.0, "8", True):
        with pytest.raises(ValueError):
            engine.open_stream(H, W, BATCH, bars=bad)
    box, n = (C.c_int32 * 4)(), C.c_longlong(0)
    with engine.open_stream(H, W, BATCH) as vs:
        lib, s = vs._lib, vs._s
        assert lib.pfnl_stream_pop_box(s, box) == -2 and lib.pfnl_stream_content_box(s, box, C.byref(n)) == -2   # mode 0
        for mode, limit in ((2, 8), (-1, 8), (1, -1), (1, 220)):
            assert lib.pfnl_stream_bars(s, mode, limit) == -1
        assert lib.pfnl_stream_bars(None, 1, 8) == -1 and lib.pfnl_stream_pop_box(s, None) == -1
        assert lib.pfnl_stream_bars(s, 1, 8) == 0
        assert lib.pfnl_stream_pop_box(s, box) == -2 and b"popped" in lib.pfnl_last_error()          # before any pop
        vs.push(_letterboxed(1)[0])
        assert lib.pfnl_stream_bars(s, 0, 0) == -2 and b"before the first frame" in lib.pfnl_last_error()
        vs.reset()
        assert lib.pfnl_stream_bars(s, 0, 0) == 0 and lib.pfnl_stream_bars(s, 1, 219) == 0


# ---- upscale --crop -------------------------------------------------------------------------------------------------------------------------
UH, UW, BAR = 32, 48, 8


def _y4m_stream(interlace, n=5):
    """(the stream with bars of BAR rows, the same stream cropped on the host beforehand) as bytes"""
    head = y4m.Y4MHeader(width=UW, height=UH, rate="25:1", interlace=interlace, siting="center", interlaced_ok=True)
    small = y4m.Y4MHeader(width=UW, height=UH - 2 * BAR, rate="25:1", interlace=interlace, siting="center", interlaced_ok=True)
    full, cropped = io.BytesIO(), io.BytesIO()
    wf, wc = y4m.Y4MWriter(full, head), y4m.Y4MWriter(cropped, small)
    for k in range(n):
        rgb = G.boxed(UH, UW, (BAR, 0, UH - 2 * BAR, UW), 255, seed=40 + k)
        frame = yuv.from_rgb(rgb, "i420", "bt601", False, "center")
        wf.write_frame(frame)
        wc.write_frame(np.concatenate([p.reshape(-1) for p in up.window_planes(frame, head, (BAR, 0, UH - 2 * BAR, UW))]))
    return full.getvalue(), cropped.getvalue()


def _upscale(engine, data, **kw):
    out, err = io.BytesIO(), io.StringIO()
    interlaced = b" It" in data.split(b"\n", 1)[0]
    n = up.upscale(y4m.Y4MReader(io.BytesIO(data), interlaced=interlaced), y4m.Y4MWriter(out), engine.open_stream, log=err, batch=BATCH, **kw)
    return n, out.getvalue(), err.getvalue()


@pytest.mark.parametrize("interlace", ["p", "t"])
def test_upscale_crops_ahead_of_the_network(engine, interlace):
    full, cropped = _y4m_stream(interlace)
    kw = {"deinterlace": "frame"} if interlace == "t" else {}
    a = up.parser().parse_args(["-", "-", "--synthetic-weights", "0", "--crop", f"{BAR},0,{UH - 2 * BAR},{UW}"])
    assert a.crop == (BAR, 0, UH - 2 * BAR, UW) and up.parser().parse_args(["-", "-", "--synthetic-weights", "0", "--crop", "auto"]).crop == "auto"
    n, want, _ = _upscale(engine, cropped, **kw)
    assert n == 5 and want.startswith(b"YUV4MPEG2 W%d H%d " % (4 * UW, 4 * (UH - 2 * BAR)))
    n, got, err = _upscale(engine, full, crop=a.crop, **kw)
    assert n == 5 and got == want and "crop" not in err                  # byte for byte the stream cropped beforehand
    n, auto, err = _upscale(engine, full, crop="auto", crop_probe=3, **kw)
    assert n == 5 and auto == want
    assert err.startswith(f"crop {BAR},0,{UH - 2 * BAR},{UW} (from 3 frames)\n")
    n, whole, _ = _upscale(engine, full, **kw)                           # and without --crop: the whole frame, bars and all
    assert whole.startswith(b"YUV4MPEG2 W%d H%d " % (4 * UW, 4 * UH))
