"""Host side of the device scores (pfnl_op_score_y): metrics.ssim_valid / metrics.sequence_scores against the project's
existing pins of the reference's own functions (tests/golden/ssim_ref.npz, utils_ref.npz), and the C-ABI hooks' argument
validation, which needs no device."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
from pfnl_amd import _capi, metrics


def _ssim_map(a, b, L=255.0):
    """The map metrics.ssim averages (modules/SSIM_Index.py:23-89), restated."""
    import scipy.ndimage
    c1, c2 = (0.01 * L) ** 2, (0.03 * L) ** 2
    w = metrics._gauss_2d()
    conv = lambda z: scipy.ndimage.convolve(z, w)                 # noqa: E731
    mu1, mu2 = conv(a), conv(b)
    s1, s2, s12 = conv(a * a) - mu1 * mu1, conv(b * b) - mu2 * mu2, conv(a * b) - mu1 * mu2
    return ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2))


def host_sums(ya, yb, sp_border):
    """[sum_d2_full, sum_d2_crop, ssim_sum_full, ssim_sum_valid] of two Y planes - what pfnl_op_score_y returns per frame."""
    d2 = (ya - yb) ** 2
    m = _ssim_map(ya, yb)
    H, W = ya.shape
    return [d2.sum(), d2[sp_border:H - sp_border, sp_border:W - sp_border].sum(), m.sum(), m[5:-5, 5:-5].sum()]


def test_ssim_valid_is_the_interior_mean_of_the_map():
    rng = np.random.default_rng(3)
    for H, W in ((11, 11), (12, 40), (37, 53)):
        a = rng.integers(0, 256, size=(H, W)).astype(np.float64)
        b = np.clip(np.round(a + rng.normal(0, 6, size=a.shape)), 0, 255)
        m = _ssim_map(a, b)
        assert metrics.ssim(a, b) == float(np.mean(m))
        assert metrics.ssim_valid(a, b) == float(np.mean(m[5:-5, 5:-5]))
    assert abs(metrics.ssim_valid(a, a) - 1.0) < 1e-12
    with pytest.raises(ValueError):
        metrics.ssim_valid(a[:10], b[:10])


def test_sequence_scores_reproduces_the_ssim_fixture():
    gd = load_golden("ssim_ref")
    for a, b, (h, w, s255, _s1) in zip(gd["a"], gd["b"], gd["hw_ssim255_ssim1"]):
        h, w = int(h), int(w)
        a, b = a[:h, :w], b[:h, :w]
        sc = metrics.sequence_scores([host_sums(a, b, 0)], h, w, sp_border=0, t_border=0)
        assert abs(sc["ssim"][0] - s255) < 1e-12 and abs(sc["ssim_mean"] - s255) < 1e-12
        assert abs(sc["ssim_valid"][0] - metrics.ssim_valid(a, b)) < 1e-12
        assert sc["psnr_y"][0] == metrics.psnr_y(a, b) or abs(sc["psnr_y"][0] - metrics.psnr_y(a, b)) < 1e-9


def test_sequence_scores_reproduces_avg_psnr_of_the_reference():
    gd = load_golden("utils_ref")
    yt = [metrics.rgb2ycbcr(metrics.to_uint8(f))[..., 0] for f in gd["vid_true"]]
    yp = [metrics.rgb2ycbcr(metrics.to_uint8(f))[..., 0] for f in gd["vid_pred"]]
    H, W = yt[0].shape
    for (sp, tb), want in (((8, 2), gd["avg_psnr"][0]), ((4, 0), gd["avg_psnr"][2])):
        sc = metrics.sequence_scores([host_sums(a, b, sp) for a, b in zip(yt, yp)], H, W, sp_border=sp, t_border=tb)
        assert abs(sc["avg_psnr"] - want) < 1e-9
        assert len(sc["psnr_y"]) == len(sc["ssim"]) == len(sc["ssim_valid"]) == len(yt)
        assert abs(sc["psnr_y_mean"] - np.mean([metrics.psnr_y(a, b) for a, b in zip(yt, yp)])) < 1e-9


def test_sequence_scores_edges():
    one = [[0.0, 0.0, 24.0 * 32.0, 14.0 * 22.0]]                    # identical frames: no error, a map of ones
    sc = metrics.sequence_scores(one * 5, 24, 32)
    assert sc["psnr_y"] == [float("inf")] * 5 and sc["avg_psnr"] == float("inf")
    assert sc["ssim"] == [1.0] * 5 and sc["ssim_valid"] == [1.0] * 5
    assert np.isnan(metrics.sequence_scores(one * 4, 24, 32)["avg_psnr"])        # t_border 2 leaves no frame of 4
    assert metrics.sequence_scores(one * 4, 24, 32, t_border=0)["avg_psnr"] == float("inf")
    empty = metrics.sequence_scores(np.zeros((0, 4)), 24, 32)
    assert empty["psnr_y"] == [] and np.isnan(empty["psnr_y_mean"]) and np.isnan(empty["avg_psnr"])


def test_score_hooks_validate_arguments_without_gpu():
    """pfnl_op_score_y / pfnl_op_score_scratch_bytes refuse bad arguments before any HIP call; the ABI version stays 4."""
    lib = _capi.load_library()
    assert lib.pfnl_version() == 4
    n = C.c_size_t(0)
    assert lib.pfnl_op_score_scratch_bytes(8, 576, 720, C.byref(n)) == 0
    tiles = -(-576 // 16) * -(-720 // 32)
    assert n.value >= 8 * tiles * 4 * 8 and n.value % 8 == 0          # at least one slot of four doubles per frame
    assert lib.pfnl_op_score_scratch_bytes(1, 11, 11, C.byref(n)) == 0 and n.value >= 32
    assert lib.pfnl_op_score_scratch_bytes(50, 2160, 3840, C.byref(n)) == 0 and n.value > 0
    assert lib.pfnl_op_score_scratch_bytes(1, 11, 11, None) == -1 and b"NULL" in lib.pfnl_last_error()
    for F, H, W in ((0, 64, 64), (-1, 64, 64), (1, 10, 64), (1, 64, 10), (1, 0, 0)):
        assert lib.pfnl_op_score_scratch_bytes(F, H, W, C.byref(n)) == -1, (F, H, W)
    dummy = C.c_void_p(16)                                            # never dereferenced: the hook returns first
    score = lambda p, t, F, H, W, b, o, s: lib.pfnl_op_score_y(p, t, F, H, W, b, o, s, None)   # noqa: E731
    for args in ((None, dummy, dummy, dummy), (dummy, None, dummy, dummy), (dummy, dummy, None, dummy), (dummy, dummy, dummy, None)):
        p, t, o, s = args
        assert score(p, t, 1, 64, 64, 8, o, s) == -1 and b"NULL" in lib.pfnl_last_error()
    assert score(dummy, dummy, 1, 10, 64, 0, dummy, dummy) == -1 and b"11" in lib.pfnl_last_error()
    assert score(dummy, dummy, 1, 64, 10, 0, dummy, dummy) == -1
    assert score(dummy, dummy, 0, 64, 64, 8, dummy, dummy) == -1
    assert score(dummy, dummy, 1, 16, 64, 8, dummy, dummy) == -1 and b"sp_border" in lib.pfnl_last_error()   # 2 * 8 >= H
    assert score(dummy, dummy, 1, 64, 16, 8, dummy, dummy) == -1
    assert score(dummy, dummy, 1, 64, 64, -1, dummy, dummy) == -1


def test_score_of_too_small_frames_is_refused_before_any_device_work(tmp_path):
    """score_video_truth on HR frames below the 11 x 11 SSIM window: ValueError, as matlab/SSIM.m refuses them."""
    from PIL import Image
    from model.pfnl import PFNL
    seq = tmp_path / "tiny"
    (seq / "truth").mkdir(parents=True)
    for i in range(2):
        Image.fromarray(np.full((10, 40, 3), 7 * i, np.uint8)).save(seq / "truth" / f"{i:04d}.png")
    with pytest.raises(ValueError, match="11 x 11"):
        PFNL().score_video_truth(str(seq), name="out")
