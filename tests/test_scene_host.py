"""The scene rule on the host (pfnl_amd/scene.py): the luma sum, the cut rule on hand-computed values, and the per-scene windows against
a brute-force split of the sequence into scenes; the session's scene calls refuse NULL without a device."""
import numpy as np
import pytest

from pfnl_amd import _capi, scene
from pfnl_amd import model as M


def _brute_force_index(sf, T, last):
    """every scene among the frames 0..last as a sequence of its own through model.sliding_windows"""
    sf = np.asarray(sf[:last + 1])
    idx = np.zeros((last + 1, T), np.int64)
    for a in np.unique(sf):
        members = np.flatnonzero(sf == a)
        assert members[0] == a and np.array_equal(members, np.arange(a, a + len(members)))   # contiguous, starting at its first frame
        idx[members] = M.sliding_windows(members, T)
    return idx


def _first_from_cuts(F, cuts):
    sf = np.zeros((F,), np.int64)
    for f in range(1, F):
        sf[f] = f if f in cuts else sf[f - 1]
    return sf


LAYOUTS = [(12, ()), (12, (1,)), (12, (11,)), (12, (1, 2)), (12, (4, 9)), (12, (5, 6, 7)), (1, ()), (2, (1,)), (5, (1, 2, 3, 4))]


@pytest.mark.parametrize("T", [3, 5, 7])
def test_scene_windows_index_equals_per_scene_sliding_windows(T):
    rng = np.random.default_rng(T)
    layouts = list(LAYOUTS)
    for _ in range(40):
        F = int(rng.integers(1, 25))
        layouts.append((F, tuple(int(c) for c in np.flatnonzero(rng.random(F) < 0.3) if c > 0)))
    for F, cuts in layouts:
        sf = _first_from_cuts(F, set(cuts))
        for last in sorted({F - 1, F // 2, 0} | {int(rng.integers(0, F))}):     # the end, the middle of a scene, the first frame
            got = scene.scene_windows_index(sf, T, last)
            assert got.shape == (last + 1, T) and got.dtype == np.int64
            assert np.array_equal(got, _brute_force_index(sf, T, last)), (F, cuts, T, last)
        assert np.array_equal(scene.scene_windows_index(sf, T), scene.scene_windows_index(sf, T, F - 1))


@pytest.mark.parametrize("T", [3, 5, 7])
def test_one_scene_gives_the_reference_windows(T):
    frames = np.arange(9)
    assert np.array_equal(frames[scene.scene_windows_index(np.zeros(9, np.int64), T)], M.sliding_windows(frames, T))


def test_luma_and_sad_on_hand_computed_values():
    px = lambda r, g, b: np.array([[[r, g, b]]], np.uint8)   # noqa: E731
    assert scene.luma_u8(px(0, 0, 0))[0, 0] == 0
    assert scene.luma_u8(px(255, 255, 255))[0, 0] == (220 * 255 + 128) >> 8 == 219
    assert scene.luma_u8(px(255, 0, 0))[0, 0] == (66 * 255 + 128) >> 8 == 66
    assert scene.luma_u8(px(0, 255, 0))[0, 0] == 128 and scene.luma_u8(px(0, 0, 255))[0, 0] == 25
    assert scene.luma_u8(px(1, 1, 1))[0, 0] == 1 and scene.luma_u8(px(0, 0, 5))[0, 0] == 0   # (348 >> 8, 253 >> 8)
    a, b = np.zeros((5, 7, 3), np.uint8), np.full((5, 7, 3), 255, np.uint8)
    assert scene.frame_sad(a, b) == scene.frame_sad(b, a) == 219 * 35 and scene.frame_sad(a, a) == 0
    assert isinstance(scene.frame_sad(a, b), int)
    b = a.copy()
    b[4, 6, 1] = 2                                            # 258 + 128 = 386 -> 1
    assert scene.frame_sad(a, b) == 1


def test_cut_rule_and_threshold_sum_on_hand_computed_values():
    assert scene.threshold_sum(10, 16, 24) == 3840
    assert scene.threshold_sum(0.3, 5, 7) == 11               # 10.5 -> 11
    assert scene.threshold_sum(255, 2, 2) == 1020
    assert scene.threshold_sum(1e-9, 16, 24) == 1             # never 0: identical frames are no cut
    for bad in (0, -1, 255.5):
        with pytest.raises(ValueError):
            scene.threshold_sum(bad, 4, 4)
    assert scene.cut_rule(5000, 100, 3840)                    # a cut: min(5000, 4900)
    assert not scene.cut_rule(100, 5000, 3840)                # the frame behind it: min(100, 4900)
    assert not scene.cut_rule(5000, 4800, 3840)               # sustained motion: min(5000, 200)
    assert scene.cut_rule(3840, 0, 3840) and not scene.cut_rule(3839, 0, 3840)   # >=, not >
    assert not scene.cut_rule(3840, 1, 3840)                  # min(3840, 3839)
    assert scene.cut_rule(9000, 5000, 3840)                   # a cut out of motion: min(9000, 4000)


def test_scene_first_from_marks_and_from_the_detector():
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, size=(3, 16, 24, 3))
    which = [0] * 4 + [1] * 5 + [2] * 3
    frames = np.stack([np.clip(base[k] + rng.integers(-2, 3, size=(16, 24, 3)), 0, 255).astype(np.uint8) for k in which])
    assert list(scene.scene_first(frames)) == [0] * 12
    assert list(scene.scene_first(frames, marks={5})) == [0] * 5 + [5] * 7
    assert list(scene.scene_first(frames, marks={0, 1, 2})) == [0, 1] + [2] * 10          # frame 0 is never a cut
    assert list(scene.scene_first(frames, threshold=10)) == [0] * 4 + [4] * 5 + [9] * 3
    assert list(scene.scene_first(frames, threshold=10, marks={2})) == [0, 0, 2, 2] + [4] * 5 + [9] * 3
    sads = scene.frame_sads(frames)
    assert sads[0] == 0 and sads[4] == scene.frame_sad(frames[4], frames[3])
    alt = np.stack([base[k % 2].astype(np.uint8) for k in range(8)])                      # every frame differs from the one before it
    assert list(scene.scene_first(alt, threshold=10)) == [0] + [1] * 7                   # ... and only the first change is a cut
    assert scene.scene_first(frames[:0]).shape == (0,)


def test_scene_calls_refuse_null_without_a_device():
    import ctypes as C
    lib = _capi.load_library()
    assert lib.pfnl_stream_scenes(None, 1, 0.0) == -1 and b"NULL" in lib.pfnl_last_error()
    assert lib.pfnl_stream_mark_cut(None) == -1 and b"NULL" in lib.pfnl_last_error()
    first, sad = C.c_longlong(0), C.c_ulonglong(0)
    assert lib.pfnl_stream_pop_info(None, C.byref(first), C.byref(sad)) == -1 and b"NULL" in lib.pfnl_last_error()
    dummy = C.c_void_p(16)                                    # never dereferenced: the hooks return first
    assert lib.pfnl_op_scene_sad_u8(dummy, dummy, 0, 4, dummy, None) == -1
    assert lib.pfnl_op_scene_sad_u8(dummy, None, 4, 4, dummy, None) == -1 and b"NULL" in lib.pfnl_last_error()
    assert lib.pfnl_op_gather_windows_u8_scenes(dummy, None, dummy, 13, 5, 0, 1, 7, 16, 24, None) == -1 and b"NULL" in lib.pfnl_last_error()
    assert lib.pfnl_op_gather_windows_u8_scenes(dummy, dummy, dummy, 13, 5, 4, 3, 7, 16, 24, None) == -1 and b"beyond" in lib.pfnl_last_error()
    assert lib.pfnl_op_gather_windows_u8_scenes(dummy, dummy, dummy, 4, 20, 10, 2, 7, 16, 24, None) == -1 and b"ring holds" in lib.pfnl_last_error()
