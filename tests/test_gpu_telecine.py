"""Inverse telecine on a real MI355X (include/pfnl_hip.h TELECINE; pfnl_amd/csrc/telecine.hip): the match and the weave at both depths in
their 16-byte, 4-byte and single-sample forms against pfnl_amd/telecine.py - counts and bytes exact -, and the session with the setting on
against a progressive RGB session pushed with telecine.frames(decode_fields(...)): for clean 3:2 material, the film itself.  No tolerance
anywhere."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import telecine_gen as G  # noqa: E402
from pfnl_amd import _capi, deinterlace, ops, synth, yuv  # noqa: E402
from pfnl_amd import packed as P  # noqa: E402
from pfnl_amd import telecine as TC  # noqa: E402
from pfnl_amd.engine import PFNLEngine  # noqa: E402
from pfnl_amd.spec import PFNLGeometry  # noqa: E402

# h x W of a field: every row index clamps (h = 1); rows of 3, 15, 51 and 66 samples - no multiple of 16, 4 or (15, 51) 2 bytes at 8 bits,
# 4-byte words at 10 bits for 66 -; h = 9: a strip boundary inside the field and a last strip one row long; h = 70 at W = 22: 1188 lanes at
# single samples - more than one workgroup of 256 adds to the sum
OP_SHAPES = [(h, w) for h in (1, 2, 3, 9) for w in (1, 5, 17, 22)] + [(70, 22)]
WORD_SHAPES = [(2, 16), (9, 32), (70, 32)]                              # rows of 48 and 96 bytes: the 16-byte form at both depths
BATCH = 2


def _cuda(a):
    a = np.ascontiguousarray(a)                                          # (torch copies int16, not uint16)
    return torch.from_numpy(a).cuda() if a.dtype == np.uint8 else torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)


def _numpy(t):
    return t.cpu().numpy() if t.dtype == torch.uint8 else t.view(torch.int16).cpu().numpy().view(np.uint16)


def _at_offset(a, off, fill):
    """``a`` in a device buffer of ``fill`` bytes, ``off`` bytes behind a 256-byte boundary, 64 bytes of ``fill`` behind it: (buffer, view)"""
    nbytes = a.size * a.itemsize
    buf = torch.full((off + nbytes + 64,), fill, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    raw = buf[off:off + nbytes]
    raw.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8)).cuda())
    view = raw if a.dtype == np.uint8 else raw.view(torch.uint16)
    return buf, view.view(a.shape)


# ---- the ops --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("maxv", [255, 1023])
@pytest.mark.parametrize("h,w", OP_SHAPES + WORD_SHAPES)
def test_the_match_counts_what_comb_count_counts(h, w, maxv):
    A, Xc, Xp = G.candidates(h, w, maxv)
    dev = [_cuda(f) for f in (A, Xc, Xp)]
    for parity in (0, 1):
        for thr in (10, 1, 255):
            want = (TC.comb_count(A, Xc, parity, thr, maxv), TC.comb_count(A, Xp, parity, thr, maxv))
            assert ops.fieldmatch(*dev, parity, thr) == want, (h, w, maxv, parity, thr)
    assert 0 < TC.comb_count(A, Xp, 0, 10, maxv) < h * w * 3 or h * w < 4   # (the content lands on both sides of the threshold)
    assert ops.fieldmatch(dev[0], dev[0], dev[0], 1) == (TC.comb_count(A, A, 1, 10, maxv),) * 2   # the fields may be one another


@pytest.mark.parametrize("maxv", [255, 1023])
@pytest.mark.parametrize("h,w", [(3, 5), (9, 22), (9, 32), (70, 22)])
def test_pointers_offset_by_one_sample(h, w, maxv):
    """every pointer one sample off a 256-byte boundary: single samples at 8 bits, and at 10 bits on rows that would allow words"""
    A, Xc, Xp = G.candidates(h, w, maxv, seed=5)
    off = A.itemsize
    held = [_at_offset(f, off, 0x5A) for f in (A, Xc, Xp)]
    views = [v for _, v in held]
    for parity in (0, 1):
        which, cc, cp = TC.match(A, Xc, Xp, parity, 10, maxv)
        assert ops.fieldmatch(*views, parity) == (cc, cp)
        want = TC.weave(A, Xc if which == "c" else Xp, parity, maxv)
        buf, out = _at_offset(np.full_like(want, 0x3C3C if maxv == 1023 else 0x3C), off, 0xA5)
        got, d = ops.telecine_frame(*views, parity, out=out)
        assert got.data_ptr() == out.data_ptr() and out.data_ptr() % 16 == off
        assert d == {"count_c": cc, "count_p": cp, "match": int(which == "p"), "post": 0}
        assert np.array_equal(_numpy(got), want), (h, w, maxv, parity)
        raw = buf.cpu().numpy()
        assert (raw[:off] == 0xA5).all() and (raw[off + want.size * want.itemsize:] == 0xA5).all()
    for (_, view), f in zip(held, (A, Xc, Xp)):                         # the fields are only read
        assert np.array_equal(_numpy(view), f)


@pytest.mark.parametrize("maxv", [255, 1023])
@pytest.mark.parametrize("h,w", OP_SHAPES + WORD_SHAPES)
def test_the_frame_hook_decides_and_weaves(h, w, maxv):
    A, Xc, Xp = G.candidates(h, w, maxv, seed=3)
    dev = [_cuda(f) for f in (A, Xc, Xp)]
    sentinel = np.full((2 * h, w, 3), 77, A.dtype)                       # stands for the deinterlaced frame a session puts there
    for parity in (0, 1):
        for order in ((0, 1, 2), (0, 2, 1)):                             # either candidate as c: both matches occur
            a, xc, xp = (A, Xc, Xp)[order[0]], (A, Xc, Xp)[order[1]], (A, Xc, Xp)[order[2]]
            which, cc, cp = TC.match(a, xc, xp, parity, 10, maxv)
            woven = TC.weave(a, xc if which == "c" else xp, parity, maxv)
            got, d = ops.telecine_frame(dev[order[0]], dev[order[1]], dev[order[2]], parity)
            assert d == {"count_c": cc, "count_p": cp, "match": int(which == "p"), "post": 0} and np.array_equal(_numpy(got), woven)
            for limit in (min(cc, cp), min(cc, cp) - 1):                 # post: flagged iff the smaller count EXCEEDS the limit
                if limit < 0:
                    continue
                got, d = ops.telecine_frame(dev[order[0]], dev[order[1]], dev[order[2]], parity, post=True, comb_limit=limit, out=_cuda(sentinel))
                flagged = min(cc, cp) > limit
                assert d["post"] == int(flagged) and d["match"] == int(which == "p")
                assert np.array_equal(_numpy(got), sentinel if flagged else woven), (h, w, maxv, parity, limit)


def test_the_hooks_refuse_by_name():
    lib = _capi.load_library()
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    ok = [p, p + 256, p + 512, 2, 2, 0, 10, p + 2048, None]
    assert lib.pfnl_op_fieldmatch_u8(*ok) == 0
    for at, value, name in ((0, None, b"A is NULL"), (1, None, b"Xc"), (2, None, b"Xp"), (3, 0, b"h must"), (4, 0, b"W must"), (5, 2, b"parity"),
                            (6, 0, b"threshold"), (6, 256, b"threshold"), (7, None, b"device words"), (7, p + 2052, b"8-byte")):
        bad = list(ok)
        bad[at] = value
        assert lib.pfnl_op_fieldmatch_u8(*bad) == -1 and name in lib.pfnl_last_error(), name
    bad = list(ok)
    bad[1] = p + 257
    assert lib.pfnl_op_fieldmatch_u10(*bad) == -1 and b"Xc" in lib.pfnl_last_error()
    frame = [p, p + 256, p + 512, 2, 2, 0, None, p + 1024, p + 2048, None]
    assert lib.pfnl_op_telecine_frame_u8(*frame) == 0
    frame[7] = None
    assert lib.pfnl_op_telecine_frame_u10(*frame) == -1 and b"out is NULL" in lib.pfnl_last_error()
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


_REF = {}


def _reference(engines, frames, H, W, key, **kw):
    """the progressive session's output for ``frames``, computed once per ``key``"""
    if key not in _REF:
        with engines[1].open_stream(H, W, BATCH, **kw) as vs:
            _REF[key] = _drive(vs, frames)
    return _REF[key]


@pytest.mark.parametrize("order", ["tff", "bff"])
@pytest.mark.parametrize("phase", range(5))
@pytest.mark.parametrize("H,W", G.SHAPES)
def test_decimate_gives_the_film_back(engines, H, W, phase, order):
    film = G.film(G.N_FILM, H, W)
    pushed = TC.pulldown(film, phase, order)
    assert len(pushed) == G.N_PUSHED
    want = _reference(engines, film, H, W, ("film", H, W))
    with engines[0].open_stream(H, W, BATCH, telecine="decimate", field_order=order) as vs:
        _same(_drive(vs, pushed, "alt" if phase % 2 else "host"), want)
        assert vs.telecine_stats() == dict(zip(("matched_c", "matched_p", "post", "dropped", "delivered"), TC.stats(pushed, "decimate", order)))
        assert vs.telecine_stats()["dropped"] == 2 and vs.telecine_stats()["post"] == 0


@pytest.mark.parametrize("order", ["tff", "bff"])
@pytest.mark.parametrize("phase", range(5))
def test_match_gives_every_pushed_frame_its_film_frame(engines, phase, order):
    H, W = G.SHAPES[phase % 2]
    film = G.film(G.N_FILM, H, W)
    pushed = TC.pulldown(film, phase, order)
    under = TC.pulldown_fields(G.N_FILM, phase)[0::2]                    # the film frame of every pushed frame's first field
    want = _reference(engines, [film[i] for i in under], H, W, ("match", H, W, phase))
    with engines[0].open_stream(H, W, BATCH, telecine="match", field_order=order) as vs:
        _same(_drive(vs, pushed, "device" if phase % 2 else "alt"), want)
        st = vs.telecine_stats()
        assert (st["matched_c"] + st["matched_p"], st["post"], st["dropped"], st["delivered"]) == (G.N_PUSHED, 0, 0, G.N_PUSHED)
        assert st["matched_p"] == TC.stats(pushed, "match", order)[1] > 0


def _with_video(H, W, maxv=255):
    pushed = TC.pulldown(G.film(G.N_FILM, H, W, maxv), 0, "tff")
    pushed[6:8] = G.video(2, H, W, maxv)                        # (behind a whole frame, ahead of a whole frame: two flagged, not three)
    return pushed


@pytest.mark.parametrize("mode", TC.MODES)
@pytest.mark.parametrize("post", [True, False])
def test_a_video_insert_is_post_processed(engines, mode, post):
    H, W = G.SHAPES[1]
    pushed = _with_video(H, W)
    par = {"post": post}
    want_frames = TC.frames(pushed, mode, "tff", post=post)
    st = TC.stats(pushed, mode, "tff", post=post)
    assert st[2] == (2 if post else 0)
    want = _reference(engines, want_frames, H, W, ("video", mode, post))
    with engines[0].open_stream(H, W, BATCH, telecine=mode, telecine_params=par) as vs:
        _same(_drive(vs, pushed, "alt"), want)
        assert tuple(vs.telecine_stats().values()) == st
        vs.reset()                                                       # the setting survives, the counts start again
        assert tuple(vs.telecine_stats().values()) == (0, 0, 0, 0, 0)
        _same(_drive(vs, pushed, "device"), want)
        assert tuple(vs.telecine_stats().values()) == st


# name -> (the keywords of the telecine session, those of the progressive RGB session, maxv, pushed frames in the pushed layout)
def _inputs(name, H, W):
    rgb = lambda maxv: TC.pulldown(G.film(G.N_FILM, H, W, maxv), 3, "bff")   # noqa: E731
    if name == "rgb10":
        kw = {"in_depth": 10, "out_format": "rgb10"}
        return kw, kw, 1023, rgb(1023)
    if name == "i420":
        return {"pixel_format": "i420"}, {"out_format": "i420"}, 255, [yuv.from_rgb(f, "i420") for f in rgb(255)]
    if name == "yuyv422":
        return ({"pixel_format": "nv12", "chroma": "422", "packing": "yuyv422", "out_format": "rgb24", "chroma_siting": "center"}, {}, 255,
                [P.from_rgb(f, "yuyv422", "bt709", False, "center") for f in rgb(255)])
    assert name == "v210"
    return ({"pixel_format": "i420", "in_depth": 10, "chroma": "422", "packing": "v210", "out_format": "i010", "out_chroma": "422"},
            {"in_depth": 10, "out_format": "i010", "out_chroma": "422"}, 1023, [P.from_rgb(f, "v210") for f in rgb(1023)])


@pytest.mark.parametrize("name,H,W", [("rgb10", 8, 12), ("rgb10", 16, 20), ("i420", 16, 20), ("yuyv422", 8, 12), ("v210", 16, 24)])
def test_every_input_family_goes_through_the_field_store(engines, name, H, W):
    kw, ref_kw, maxv, pushed = _inputs(name, H, W)
    decode = {"in_depth": kw.get("in_depth", 8), "chroma": kw.get("chroma", "420"), "packing": kw.get("packing"),
              "siting": kw.get("chroma_siting", "left")}
    rgb = [deinterlace.decode_fields(f, kw.get("pixel_format", "rgb24"), H, W, **decode) for f in pushed]
    frames = TC.frames(rgb, "decimate", "bff", maxv=maxv)
    assert len(frames) == G.N_FILM
    want = _reference(engines, frames, H, W, ("family", name, H, W), **ref_kw)
    with engines[0].open_stream(H, W, BATCH, telecine="decimate", field_order="bff", **kw) as vs:
        for how in ("alt", "device"):
            _same(_drive(vs, pushed, how), want)
            assert tuple(vs.telecine_stats().values()) == TC.stats(rgb, "decimate", "bff", maxv=maxv)
            vs.reset()


@pytest.mark.parametrize("at", [1, 6, 9])
def test_a_mark_on_a_dropped_frame_lands_on_the_next_delivered_one(engines, at):
    """phase 0: pushed frames 1 and 6 repeat their predecessors and are dropped; a mark on 1 lands on pushed frame 2 = delivered frame 1, one
    on 6 on pushed 7 = delivered 5; a mark on pushed frame 9 (kept) lands on delivered frame 7"""
    H, W = G.SHAPES[0]
    film = G.film(G.N_FILM, H, W)
    pushed = TC.pulldown(film, 0, "tff")
    m, _ = TC.matched_frames(pushed, "tff")
    _, dropped, marks = TC.decimate(m, [i == at for i in range(len(pushed))])
    assert dropped == [1, 6]
    lands = marks.index(True)
    assert lands == {1: 1, 6: 5, 9: 7}[at]
    with engines[1].open_stream(H, W, BATCH, scene_cut="manual") as vs:
        want = _drive(vs, film, before=lambda i: vs.mark_cut() if i == lands else None)
        assert vs.cuts == [lands]
    with engines[0].open_stream(H, W, BATCH, scene_cut="manual", telecine="decimate") as vs:
        for how in ("host", "device"):
            _same(_drive(vs, pushed, how, before=lambda i: vs.mark_cut() if i == at else None), want)
            assert vs.cuts == [lands]
            vs.reset()


@pytest.mark.parametrize("n", [1, 3, 5, 7])
def test_the_end_in_mid_cycle_delivers_the_cycle_whole(engines, n):
    H, W = G.SHAPES[0]
    pushed = TC.pulldown(G.film(G.N_FILM, H, W), 0, "tff")[:n]
    frames = TC.frames(pushed, "decimate", "tff")
    assert len(frames) == TC.deliverable("decimate", n, True) == {1: 1, 3: 3, 5: 4, 7: 6}[n]
    want = _reference(engines, frames, H, W, ("end", n))
    with engines[0].open_stream(H, W, BATCH, telecine="decimate") as vs:
        _same(_drive(vs, pushed, "alt"), want)
        vs.reset()
        _same(_drive(vs, pushed, "host"), want)                          # reset, then a second sequence: cycles count from the reset


def test_reset_in_mid_cycle_forgets_the_cycle(engines):
    H, W = G.SHAPES[0]
    film = G.film(G.N_FILM, H, W)
    pushed = TC.pulldown(film, 4, "tff")
    want = _reference(engines, film, H, W, ("film", H, W))
    with engines[0].open_stream(H, W, BATCH, scene_cut="manual", telecine="decimate") as vs:
        for f in pushed[2:9]:
            vs.push(f)
        vs.mark_cut()                                                    # a pending mark is forgotten
        vs.reset()
        _same(_drive(vs, pushed), want)
        assert vs.cuts == []


def test_the_bound_refuses_a_push_and_changes_nothing(engines):
    H, W = G.SHAPES[0]
    film = G.film(16, H, W)
    pushed = TC.pulldown(film, 0, "tff")
    assert len(pushed) == 20
    want = _reference(engines, film, H, W, ("film16", H, W))
    with engines[0].open_stream(H, W, BATCH, telecine="decimate") as vs:
        lib, s = vs._lib, vs._handle()
        push = lambda f: lib.pfnl_stream_push(s, f.ctypes.data_as(C.c_void_p), 0)   # noqa: E731
        i = 0
        while i < len(pushed) and push(pushed[i]) == 0:                  # no pops
            i += 1
        assert 0 < i < len(pushed) and b"pop first" in lib.pfnl_last_error()
        assert i % 5 == 0                                                # the push that completes a cycle: four ring frames or none
        ready, stats = vs.ready(), vs.telecine_stats()
        assert ready == 2 * BATCH
        assert push(pushed[i]) == -2 and vs.ready() == ready and vs.telecine_stats() == stats   # the frame was not stored, no counter moved
        got = vs.pop_ready()
        assert [k for k, _ in got] == list(range(ready))
        for f in pushed[i:]:                                             # the refused frame again, and the rest: the same bytes
            got += vs.push(f)
            got += vs.pop_ready()
        got += vs.end()
        _same(got, want)


def test_refusals(engines):
    H, W = G.SHAPES[0]
    for bad in ({"telecine": "both"}, {"telecine": 1}, {"telecine": "match", "field_order": "top"}, {"telecine": "match", "interlaced": "frame"},
                {"telecine": "decimate", "pixel_format": "i420", "H": 18}, {"telecine": "match", "H": 9},
                {"telecine": "match", "telecine_params": {"threshold": 0}}, {"telecine": "match", "telecine_params": {"limit": 3}}):
        with pytest.raises(ValueError):                                  # refused before anything touches the engine
            engines[0].open_stream(bad.pop("H", H), W, BATCH, **bad)
    with engines[0].open_stream(H, W, BATCH) as vs:
        lib, s = vs._lib, vs._s
        for mode, order in ((3, 0), (-1, 0), (1, 2)):
            assert lib.pfnl_stream_telecine(s, mode, order, None) == -1
        par = _capi.pfnl_telecine_params(300, 1, -1)
        assert lib.pfnl_stream_telecine(s, 1, 0, C.byref(par)) == -1 and b"threshold" in lib.pfnl_last_error()
        assert lib.pfnl_stream_interlace(s, 1, 0) == 0
        assert lib.pfnl_stream_telecine(s, 1, 0, None) == -1 and b"exclusive" in lib.pfnl_last_error()
        assert lib.pfnl_stream_telecine(s, 0, 0, None) == 0              # off beside it is no contradiction
        assert lib.pfnl_stream_interlace(s, 0, 0) == 0 and lib.pfnl_stream_telecine(s, 2, 1, None) == 0
        assert lib.pfnl_stream_interlace(s, 2, 0) == -1 and b"exclusive" in lib.pfnl_last_error()
        vs.telecine = "decimate"
        vs.push(G.film(1, H, W)[0])                                      # held: no ring frame yet, and the settings are fixed all the same
        assert lib.pfnl_stream_telecine(s, 0, 0, None) == -2 and b"before the first frame" in lib.pfnl_last_error()
        vs.reset()
        assert lib.pfnl_stream_telecine(s, 0, 0, None) == 0
    with engines[0].open_stream(18, W, BATCH, pixel_format="i420") as vs:   # 4:2:0 and H = 18: whichever call comes second refuses
        assert vs._lib.pfnl_stream_telecine(vs._s, 1, 0, None) == -1 and b"multiple of 4" in vs._lib.pfnl_last_error()
        assert vs._lib.pfnl_stream_chroma_format(vs._s, 1, 1) == 0 and vs._lib.pfnl_stream_telecine(vs._s, 1, 0, None) == 0
        assert vs._lib.pfnl_stream_chroma_format(vs._s, 0, 0) == -1 and b"multiple of 4" in vs._lib.pfnl_last_error()
    with engines[0].open_stream(H, W, 1) as vs:                          # a batch of 1 never holds a cycle's four frames
        assert vs._lib.pfnl_stream_telecine(vs._s, 2, 0, None) == -1 and b"larger batch" in vs._lib.pfnl_last_error()
        assert vs._lib.pfnl_stream_telecine(vs._s, 1, 0, None) == 0


def test_with_the_setting_off_the_session_is_todays(engines):
    H, W = G.SHAPES[0]
    film = G.film(G.N_FILM, H, W)
    want = _reference(engines, film, H, W, ("film", H, W))
    with engines[0].open_stream(H, W, BATCH) as vs:
        assert vs._lib.pfnl_stream_telecine(vs._s, 2, 0, None) == 0 and vs._lib.pfnl_stream_telecine(vs._s, 0, 0, None) == 0
        _same(_drive(vs, film, "alt"), want)                             # turned on and off again: what a session that never called it delivers
        assert tuple(vs.telecine_stats().values()) == (0, 0, 0, 0, 0)
    with engines[0].open_stream(H, W, BATCH, interlaced="frame") as vs:  # ... and the deinterlacer beside it is what it was
        woven = TC.pulldown(film, 1, "tff")
        got = _drive(vs, woven)
    with engines[1].open_stream(H, W, BATCH) as vs:
        _same(got, _drive(vs, deinterlace.frames(woven, "tff", "frame")))
