"""Scenes in the streaming session on a real MI355X (include/pfnl_hip.h pfnl_stream_scenes / mark_cut / pop_info; pfnl_amd/scene.py is the
rule): the luma sum is exact, the scene-aware gather names the frames of scene_windows_index bit for bit, a session with cuts delivers
the bytes of its scenes run as sequences of their own, the detector finds what the numpy rule finds, and the session's bounds, reset and
range fence behave as they do without scenes."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfnl_amd import model as M  # noqa: E402
from pfnl_amd import _capi, ops, scene, synth  # noqa: E402
from pfnl_amd.engine import PFNLEngine  # noqa: E402
from pfnl_amd.spec import PFNLGeometry  # noqa: E402

GEOM = PFNLGeometry(num_block=1)
T = GEOM.num_frames
H, W = 16, 24


def _engine_with(w, precision="fp32"):
    e = PFNLEngine(GEOM, device=0)
    e.load_weights(w)
    if precision != "fp32":
        e.set_option("precision", precision)
    return e


def _frames_u8(F, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(F, h, w, 3), dtype=np.uint8)


def _scenes_u8(lengths, seed, h=H, w=W):
    """one fixed random base image per scene + per-frame noise in [-2, 2], clipped"""
    rng = np.random.default_rng(seed)
    out = []
    for n in lengths:
        base = rng.integers(0, 256, size=(h, w, 3))
        out += [np.clip(base + rng.integers(-2, 3, size=(h, w, 3)), 0, 255).astype(np.uint8) for _ in range(n)]
    return np.stack(out)


def _stream_all(vs, frames, marks=(), device=False):
    """push one frame at a time (mark_cut before the frames in `marks`), pop one at a time: ([frame], [last_info]) in delivery order"""
    got, infos = [], []

    def drain():
        while True:
            item = vs.pop()
            if item is None:
                return
            assert item[0] == len(got)
            got.append(item[1].cpu().numpy() if device else item[1])
            infos.append(vs.last_info)

    for k, f in enumerate(frames):
        if k in marks:
            vs.mark_cut()
        assert vs.push(torch.from_numpy(f).cuda() if device else f) == []      # (everything deliverable was popped before)
        drain()
    _capi.check(vs._lib.pfnl_stream_end(vs._s))                                 # (vs.end() would pop the rest in one go)
    drain()
    return np.stack(got), infos


def _explicit(eng, frames_u8, idx, batch):
    """host-built windows through eng.forward and ops.quantise_u8 on the session's batch partition: [F,sH,sW,3] uint8"""
    win = (frames_u8 / 255.).astype(np.float32)[idx]
    outs = []
    for first in range(0, len(idx), batch):
        x = torch.from_numpy(np.ascontiguousarray(win[first:first + batch])).cuda()
        outs.append(ops.quantise_u8(eng.forward(x))[:, 0].cpu().numpy())
    return np.concatenate(outs)


# ---- 1. the luma sum ------------------------------------------------------------------------------------------------------------------
# H*W*3 = 105 (odd pixel count: a byte tail behind the 12-byte groups), 180 (4-byte reads), 1152 (16-byte reads), 5100 (two blocks)
@pytest.mark.parametrize("h,w", [(5, 7), (6, 10), (16, 24), (34, 50)])
def test_scene_sad_is_exact(h, w):
    rng = np.random.default_rng(h * w)
    a, b = _frames_u8(2, h, w, seed=h + w)
    zeros, ones = np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8)
    last_px = [a.copy() for _ in range(3)]
    for ch in range(3):
        last_px[ch][h - 1, w - 1, ch] ^= 0x80                                   # one byte of the last pixel
    pairs = [(a, b), (b, a), (a, a), (zeros, ones), (ones, zeros)] + [(a, p) for p in last_px]
    pairs.append((rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8), rng.integers(0, 3, size=(h, w, 3), dtype=np.uint8)))
    for x, y in pairs:
        want = scene.frame_sad(x, y)
        assert ops.scene_sad_u8(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()) == want
    assert scene.frame_sad(zeros, ones) == 219 * h * w and scene.frame_sad(a, a) == 0
    assert all(scene.frame_sad(a, p) > 0 for p in last_px[:2])                  # (R and G: a change of 128 always moves the luma)
    # frames that start at an odd address: the single-byte reads
    n = h * w * 3
    buf = torch.from_numpy(np.concatenate([[0], a.ravel(), [0, 0], b.ravel()]).astype(np.uint8)).cuda()
    assert ops.scene_sad_u8(buf[1:1 + n].view(h, w, 3), buf[n + 3:2 * n + 3].view(h, w, 3)) == scene.frame_sad(a, b)


# ---- 2. the scene-aware gather ----------------------------------------------------------------------------------------------------------
LAYOUTS = [("left of the centre", {18}), ("right of the centre", {22}), ("both sides", {19, 22}), ("at the centre", {20}),
           ("a one-frame scene", {20, 21}), ("cuts at every window of the batch", {20, 21, 22, 23}), ("none", set())]


@pytest.mark.parametrize("Tn", [3, 5, 7])
@pytest.mark.parametrize("h,w", [(6, 10), (16, 24)])        # 4-byte reads and 16-byte reads
def test_gather_windows_u8_scenes_equals_the_host_rule(Tn, h, w):
    F, cap = 40, 13
    seq = _frames_u8(F, h, w, 200 + Tn)
    for name, cuts in LAYOUTS:
        sf = np.zeros((F,), np.int64)
        for f in range(1, F):
            sf[f] = f if f in cuts else sf[f - 1]
        for last, first, count in [(30, 20, 4),                # the interior, a wrapped ring (first > cap)
                                   (21, 20, 2),                # `last` inside the look-ahead: the right clamp is min(scene end, last)
                                   (39, 17, 6)]:
            lo, hi = max(0, first - Tn // 2), min(last, first + count - 1 + Tn // 2)
            assert hi - lo + 1 <= cap and first > cap
            ring = 255 - seq[:cap].copy()                      # slots the windows do not name hold other bytes ...
            table = np.full((cap,), 12345, np.int64)           # ... and other scenes
            for f in range(lo, hi + 1):
                ring[f % cap] = seq[f]
                table[f % cap] = sf[f]
            idx = scene.scene_windows_index(sf, Tn, last)[first:first + count]
            want = (seq[idx] / 255.).astype(np.float32)
            d_ring = torch.from_numpy(ring).cuda()
            got = ops.gather_windows_u8_scenes(d_ring, torch.from_numpy(table).cuda(), last, first, count, Tn).cpu().numpy()
            assert got.dtype == np.float32 and got.shape == want.shape == (count, Tn, h, w, 3)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, Tn, h, w, last, first, count)   # bit for bit
            if not cuts:
                plain = ops.gather_windows_u8(d_ring, last, first, count, Tn).cpu().numpy()
                assert np.array_equal(got.view(np.uint32), plain.view(np.uint32))


# ---- 3. a session with marked cuts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("marks", [(5,), (1, 2), (4, 9), (11,)])
def test_marked_session_equals_its_scenes_run_alone(marks, precision):
    F = 12
    w = synth.synthetic_weights(GEOM, seed=0)
    eng, eng2 = _engine_with(w, precision), _engine_with(w, precision)
    frames = _frames_u8(F, H, W, seed=sum(marks))
    sf = scene.scene_first(frames, marks=marks)
    idx = scene.scene_windows_index(sf, T)
    # batch 1: the concatenation of separate sessions, one per scene
    with eng.open_stream(H, W, 1, scene_cut="manual") as vs:
        got, infos = _stream_all(vs, frames, marks)
        assert vs.cuts == list(marks)
    alone = []
    for a, b in zip((0,) + marks, marks + (F,)):
        with eng2.open_stream(H, W, 1) as vs:
            alone.append(_stream_all(vs, frames[a:b])[0])
    assert got.shape == (F, 4 * H, 4 * W, 3) and got.dtype == np.uint8
    assert np.array_equal(got, np.concatenate(alone))
    assert [i[0] for i in infos] == list(sf)
    assert [i[1] for i in infos] == scene.frame_sads(frames)                   # marks only: the sums are reported all the same
    # batches: the explicit path on the same partition
    for batch in (3, 4):
        with eng.open_stream(H, W, batch, scene_cut="manual") as vs:
            got, infos = _stream_all(vs, frames, marks)
            assert vs.cuts == list(marks) and [i[0] for i in infos] == list(sf)
        assert np.array_equal(got, _explicit(eng2, frames, idx, batch)), batch
    assert eng.get_option("precision") == precision and eng.get_option("strict_fp32") == "off"
    eng.close()
    eng2.close()


def test_device_frames_give_the_same_bytes_and_may_alternate_with_host_frames():
    eng = _engine_with(synth.synthetic_weights(GEOM, seed=0))
    frames, marks = _frames_u8(12, H, W, seed=5), (4, 9)
    with eng.open_stream(H, W, 3, scene_cut=200.0) as vs:                       # (random frames: a mean difference near 60, no detection)
        host, hinfo = _stream_all(vs, frames, marks)
        assert vs.cuts == list(marks)
        vs.reset()
        dev, dinfo = _stream_all(vs, frames, marks, device=True)
        assert vs.cuts == list(marks)
        vs.reset()
        mixed = []                                                             # host and device pushes in one sequence: two streams
        for k, f in enumerate(frames):
            if k in marks:
                vs.mark_cut()
            mixed += vs.push(torch.from_numpy(f).cuda() if k % 3 == 1 else f)
        mixed += vs.end()
        assert vs.cuts == list(marks)
    assert np.array_equal(dev, host) and dinfo == hinfo
    assert [i for i, _ in mixed] == list(range(12))
    assert np.array_equal(np.stack([f if isinstance(f, np.ndarray) else f.cpu().numpy() for _, f in mixed]), host)
    assert [i[1] for i in hinfo] == scene.frame_sads(frames)
    eng.close()


# ---- 4. the detector --------------------------------------------------------------------------------------------------------------------------
def test_detector_finds_the_placed_cuts():
    frames = _scenes_u8((5, 4, 5), seed=11)
    sf = scene.scene_first(frames, threshold=10)
    assert list(sf) == [0] * 5 + [5] * 4 + [9] * 5                             # the numpy rule: exactly the two placed cuts
    sads = scene.frame_sads(frames)
    w = synth.synthetic_weights(GEOM, seed=0)
    eng, eng2 = _engine_with(w), _engine_with(w)
    with eng.open_stream(H, W, 3, scene_cut=10) as vs:
        got, infos = _stream_all(vs, frames)
        assert vs.cuts == [5, 9]
    assert infos == [(int(a), s) for a, s in zip(sf, sads)]
    assert np.array_equal(got, _explicit(eng2, frames, scene.scene_windows_index(sf, T), 3))
    eng.close()
    eng2.close()


def test_detector_on_alternating_images_fires_once():
    a, b = _frames_u8(2, H, W, seed=12)
    frames = np.stack([a, b] * 5)
    sf = scene.scene_first(frames, threshold=10)
    sads = scene.frame_sads(frames)
    assert len(set(sf)) <= 2
    eng = _engine_with(synth.synthetic_weights(GEOM, seed=0))
    with eng.open_stream(H, W, 4, scene_cut=10) as vs:
        _, infos = _stream_all(vs, frames)
        assert vs.cuts == [int(f) for f in np.flatnonzero(sf == np.arange(10)) if f > 0] and len(vs.cuts) <= 1
    assert infos == [(int(x), s) for x, s in zip(sf, sads)]
    eng.close()


def test_one_scene_with_a_threshold_gives_the_bytes_of_a_plain_session():
    frames = _scenes_u8((9,), seed=13)
    assert not scene.scene_first(frames, threshold=10).any()
    eng = _engine_with(synth.synthetic_weights(GEOM, seed=0))
    with eng.open_stream(H, W, 3, scene_cut=10) as vs:
        got, infos = _stream_all(vs, frames)
        assert vs.cuts == [] and [i[0] for i in infos] == [0] * 9
    with eng.open_stream(H, W, 3) as vs:
        plain, pinfos = _stream_all(vs, frames)
        assert vs.cuts == [] and pinfos == [(0, 0)] * 9                        # scenes off: nothing is computed
    assert np.array_equal(got, plain)
    eng.close()


# ---- 5. state ---------------------------------------------------------------------------------------------------------------------------------
def test_scene_calls_and_the_session_state():
    eng = _engine_with(synth.synthetic_weights(GEOM, seed=0))
    lib = eng._lib
    frames = _frames_u8(12, H, W, seed=6)
    first, sad = C.c_longlong(-1), C.c_ulonglong(7)
    with eng.open_stream(H, W, 2) as vs:                                        # scenes off
        assert lib.pfnl_stream_mark_cut(vs._s) == -2 and b"scenes are off" in lib.pfnl_last_error()
        for bad_mode, thr in ((3, 1.0), (-1, 1.0), (2, 0.0), (2, 255.5), (2, -3.0), (2, float("nan"))):
            assert lib.pfnl_stream_scenes(vs._s, bad_mode, thr) == -1
        assert lib.pfnl_stream_scenes(vs._s, 2, 255.0) == 0 and lib.pfnl_stream_scenes(vs._s, 0, 0.0) == 0   # settable until a frame is in
        assert lib.pfnl_stream_pop_info(vs._s, C.byref(first), C.byref(sad)) == -2                            # before any pop
        vs.push(frames[0])
        assert lib.pfnl_stream_scenes(vs._s, 1, 0.0) == -2 and b"before the first frame" in lib.pfnl_last_error()
        assert lib.pfnl_stream_mark_cut(vs._s) == -2                            # still off
        for f in frames[1:5]:
            vs.push(f)                                                          # the fifth frame launches the first batch
        assert vs.pop() is not None
        assert lib.pfnl_stream_pop_info(vs._s, C.byref(first), C.byref(sad)) == 0 and (first.value, sad.value) == (0, 0)
        vs.reset()
        assert lib.pfnl_stream_pop_info(vs._s, C.byref(first), C.byref(sad)) == -2
        assert lib.pfnl_stream_scenes(vs._s, 1, 0.0) == 0                       # the next sequence has no frame yet
        assert lib.pfnl_stream_mark_cut(vs._s) == 0
    with pytest.raises(ValueError):
        eng.open_stream(H, W, 2, scene_cut="auto")
    with eng.open_stream(H, W, 2) as vs:                                        # ... and the refused open left no session behind
        pass
    eng.close()


def test_reset_keeps_the_mode_and_clears_marks_and_cuts():
    w = synth.synthetic_weights(GEOM, seed=0)
    eng, eng2 = _engine_with(w), _engine_with(w)
    a, b = _frames_u8(9, H, W, seed=7), _frames_u8(8, H, W, seed=8)
    with eng.open_stream(H, W, 2, scene_cut="manual") as vs:
        vs.mark_cut()                                                           # before the first frame: nothing to mark
        for k, f in enumerate(a):
            if k == 3:
                vs.mark_cut()
            vs.push(f)                                                          # three batches of A launched, two delivered, one never popped
        assert vs.cuts == [3] and vs.ready() > 0
        vs.mark_cut()                                                           # pending when the sequence is dropped
        vs.reset()
        assert vs.cuts == [] and vs.last_info is None and vs.ready() == 0
        second, info2 = _stream_all(vs, b, marks=(4,))                          # the mode is still "manual"
        assert vs.cuts == [4]
    with eng2.open_stream(H, W, 2, scene_cut="manual") as vs:
        fresh, info1 = _stream_all(vs, b, marks=(4,))
    assert np.array_equal(second, fresh) and info2 == info1
    assert [i[0] for i in info2] == [0] * 4 + [4] * 4
    eng.close()
    eng2.close()


def test_the_undelivered_bound_with_scenes_on():
    """test_readiness_and_the_undelivered_bound's walk at batch 1 with a cut in it; a refused push keeps its mark for the accepted one."""
    eng = _engine_with(synth.synthetic_weights(GEOM, seed=0))
    lib = eng._lib
    frames = _frames_u8(12, H, W, seed=6)
    k = T // 2 + 3
    marks = (2, k + 2)
    want = _explicit(eng, frames[:9], scene.scene_windows_index(scene.scene_first(frames[:9], marks=marks), T), 1)
    raw_push = lambda vs, f: lib.pfnl_stream_push(vs._s, f.ctypes.data_as(C.c_void_p), 0)   # noqa: E731
    with eng.open_stream(H, W, 1, scene_cut="manual") as vs:
        for j in range(T // 2):
            if j in marks:
                vs.mark_cut()
            assert raw_push(vs, frames[j]) == 0 and vs.ready() == 0 and vs.pop() is None
        for j in range(T // 2, T // 2 + 3):                                                   # then one per push
            assert raw_push(vs, frames[j]) == 0 and vs.ready() == 1
            i, f = vs.pop()
            assert i == j - T // 2 and np.array_equal(f, want[i]) and vs.ready() == 0
        assert raw_push(vs, frames[k]) == 0 and vs.ready() == 1
        assert raw_push(vs, frames[k + 1]) == 0 and vs.ready() == 2                           # 2 * batch undelivered frames
        vs.mark_cut()
        assert raw_push(vs, frames[k + 2]) == -2 and b"pop first" in lib.pfnl_last_error()    # PFNL_ERR_STATE, nothing changed
        assert vs.ready() == 2
        i, f = vs.pop()
        assert i == 3 and np.array_equal(f, want[3])
        assert raw_push(vs, frames[k + 2]) == 0 and vs.ready() == 2                           # the refused frame, now accepted: a cut
        assert lib.pfnl_stream_end(vs._s) == 0 and vs.ready() == 5
        rest = vs.pop_ready()
        assert [i for i, _ in rest] == [4, 5, 6, 7, 8] and vs.ready() == 0 and vs.pop() is None
        assert np.array_equal(np.stack([f for _, f in rest]), want[4:])
        assert vs.cuts == list(marks) and vs.last_info[0] == k + 2
    eng.close()


# ---- 6. the range fence ---------------------------------------------------------------------------------------------------------------------
def test_session_with_a_cut_recomputes_out_of_range_batches():
    """The weights of test_session_recomputes_out_of_range_batches (a numeric overflow of binary16 operands that the library fences).  A
    mark at frame 3, batches 3, 3, 1: the flagged batches are gathered again from the ring with the same scene table, and every frame
    equals the strict engine's on the per-scene windows."""
    lr_u8 = _frames_u8(7, 12, 20, seed=21)
    w = synth.synthetic_weights(GEOM, seed=1)
    w["nlvsr/conv0/kernel"] = (w["nlvsr/conv0/kernel"] * 4e5).astype(np.float32)
    w["nlvsr/convmerge2/kernel"] = (w["nlvsr/convmerge2/kernel"] * 1e-6).astype(np.float32)
    eng = _engine_with(w)
    was = eng.get_option("strict_fp32")
    with eng.open_stream(12, 20, 3, scene_cut="manual") as vs:
        got, infos = _stream_all(vs, lr_u8, marks=(3,))
        assert vs.cuts == [3] and [i[0] for i in infos] == [0, 0, 0, 3, 3, 3, 3]
        assert eng.get_option("strict_fp32") == was                 # end + the last pop have put it back already
    strict = _engine_with(w)
    strict.set_option("strict_fp32", "on")
    idx = scene.scene_windows_index(scene.scene_first(lr_u8, marks=(3,)), T)
    sr = strict.forward(np.ascontiguousarray((lr_u8 / 255.).astype(np.float32)[idx]))
    assert np.isfinite(sr).all()
    assert np.array_equal(got, M.quantise(sr[:, 0]))
    assert eng.get_option("strict_fp32") == was == "off" and eng.get_option("precision") == "fp32" and eng.range_flagged() is False
    eng.close()
    strict.close()
