"""The session's input route on a real MI355X (pfnl_amd/csrc/stream_route.h InRoute; capi_stream.hip decode_surface, stage_host): every
input setting pushed four ways - the tight frame from the host and from the device, its planes in pitched buffers on the host and on the
device - pops the same bytes, and they are those of a progressive RGB session pushed with the host rule's decode of the same frames; once
progressive, once with interlaced="frame".  Byte for byte, no tolerance anywhere."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import test_gpu_deinterlace as D  # noqa: E402  (its shapes and helpers: H, W, BATCH, F = 16, 24, 2, 5, one block)
from pfnl_amd import depth10, surface, yuv  # noqa: E402
from pfnl_amd import packed as P  # noqa: E402
from pfnl_amd.stream import pushed_format  # noqa: E402
from test_gpu_deinterlace import H, W, BATCH, engines  # noqa: E402,F401

SETTINGS = ["rgb24", "rgb10", "nv12", "i420", "p010", "nv12-422", "i010-444", "yuyv422", "bgra", "x2rgb10", "v210"]
WAYS = ("host", "device", "host planes", "device planes")


# name -> (the keywords of the session under test, those of the progressive RGB session, maxv, frames in the pushed layout)
def _inputs(name):
    if name == "nv12":
        return {"pixel_format": "nv12"}, {"out_format": "nv12"}, 255, [yuv.from_rgb(f, "nv12") for f in D._rgb(255)]
    if name == "p010":
        return ({"pixel_format": "nv12", "in_depth": 10, "out_format": "p010"}, {"in_depth": 10, "out_format": "p010"}, 1023,
                [depth10.from_rgb10(f, "p010") for f in D._rgb(1023)])
    if name == "i010-444":
        return ({"pixel_format": "i420", "in_depth": 10, "chroma": "444", "out_format": "i010"}, {"in_depth": 10, "out_format": "i010", "out_chroma": "444"},
                1023, [depth10.from_rgb10(f, "i010", "bt709", False, "left", "444") for f in D._rgb(1023)])
    if name == "bgra":
        return {"packing": "bgra"}, {}, 255, [P.from_rgb(f, "bgra") for f in D._rgb(255)]
    if name == "x2rgb10":
        return ({"in_depth": 10, "packing": "x2rgb10", "out_format": "rgb10"}, {"in_depth": 10, "out_format": "rgb10"}, 1023,
                [P.from_rgb(f, "x2rgb10") for f in D._rgb(1023)])
    return D._inputs(name)


def _decode(frame, kw):
    """the host rule's RGB of one pushed progressive frame (what pfnl_amd/deinterlace.py decode_fields does per field)"""
    dk = D._decode_kw(kw)
    fmt, depth, chroma, packing = dk["pixel_format"], dk["in_depth"], dk["chroma"], dk["packing"]
    rest = (dk["matrix"], dk["full_range"], dk["siting"])
    if packing is not None:
        return P.to_rgb(frame, packing, H, W, *rest)
    if fmt == "rgb24":
        return depth10.values10(frame, "rgb10") if depth == 10 else frame
    if depth == 10:
        return depth10.to_rgb10(frame, "p010" if fmt == "nv12" else "i010", H, W, *rest, chroma)
    return yuv.to_rgb(frame, fmt, H, W, *rest, chroma)


def _pitched(frame, kw):
    """the frame's planes in pitched host buffers - 20 bytes behind a row of the first plane, 10 behind one of the others: no pitch is a
    multiple of 16, each is one of the plane's alignment - and what surface.views needs to find them"""
    dk = D._decode_kw(kw)
    fmt, chroma, packing = pushed_format(dk["pixel_format"], dk["in_depth"]), dk["chroma"], dk["packing"]
    if packing is not None:
        planes = [np.asarray(frame).reshape(P.frame_shape(packing, H, W))[:, :P.row_bytes(packing, W)]]
    else:
        planes = surface.split(frame, fmt, H, W, chroma)
    pitches = [p.shape[1] * p.dtype.itemsize + (10 if k else 20) for k, p in enumerate(planes)]
    assert all(v % 16 for v in pitches)
    return surface.embed(planes, pitches, 0x3C), (fmt, H, W, chroma, packing)


def _drive(vs, frames, way, kw):
    got = []
    for f in frames:
        if way == "host":
            got += vs.push(f)
        elif way == "device":
            got += vs.push(D._cuda(np.array(f)))
        else:
            bufs, layout = _pitched(f, kw)
            if way == "device planes":
                bufs = [torch.from_numpy(b).cuda() for b in bufs]
            got += vs.push_planes(*surface.views(bufs, *layout))
        got += vs.pop_ready()
    got += vs.end()
    return [(i, D._numpy(f) if torch.is_tensor(f) else f) for i, f in got]


@pytest.mark.parametrize("interlaced", [None, "frame"])
@pytest.mark.parametrize("name", SETTINGS)
def test_four_ways_in_pop_the_same_bytes(engines, name, interlaced):  # noqa: F811
    kw, ref_kw, maxv, pushed = _inputs(name)
    frames = D._progressive(kw, pushed, maxv, "tff", "frame") if interlaced else [_decode(f, kw) for f in pushed]
    assert len(frames) == D.F
    with engines[1].open_stream(H, W, BATCH, **ref_kw) as vs:
        want = D._drive(vs, frames)
    assert len(want) == D.F
    with engines[0].open_stream(H, W, BATCH, interlaced=interlaced, **kw) as vs:
        for way in WAYS:
            D._same(_drive(vs, pushed, way, kw), want)
            vs.reset()                                                   # the setting survives
