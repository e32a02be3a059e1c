"""pfnl_op_score_y (Y-channel PSNR / SSIM sums on the device) against pfnl_amd.metrics on a real MI355X, and the harness'
scoring path (PFNL.score_video_truth / score_videos) against the same metrics applied to the PNGs it wrote.

Tolerances, per frame (the bounds tests/test_host.py holds `metrics` itself to against the reference: 1e-12 / 1e-10 / 1e-9):
|SSIM - metrics.ssim| and |ssim_valid - metrics.ssim_valid| <= 1e-10, |PSNR_Y - metrics.psnr_y| <= 1e-9 dB,
|avg_psnr - metrics.avg_psnr| <= 1e-9 dB.  A numpy fp64 restatement of the kernel's separable form differs from metrics.ssim
by at most 7.8e-14 (constant 0 against constant 255; 3e-16 elsewhere); the GPU adds another summation order and FMA
contraction, each of that size."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfnl_amd import metrics, ops, synth  # noqa: E402
from pfnl_amd.spec import PFNLGeometry  # noqa: E402

SSIM_TOL, PSNR_TOL = 1e-10, 1e-9
SIZES = [(11, 11), (12, 40), (37, 53), (144, 180), (576, 720)]
CONTENT = ["identical", "corner pixel", "random bytes", "noise 2", "noise 6", "noise 20", "pixel (5,5)", "pixel (4,4)", "0 against 255"]


def _smooth(rng, H, W):
    y, x = np.mgrid[0:H, 0:W]
    ph = rng.random(3) * 6.28
    f = np.stack([127.5 + 100.0 * np.sin(x / 9.0 + p) * np.cos(y / 7.0 + 2 * p) for p in ph], axis=-1)
    return np.clip(np.round(f), 0, 255).astype(np.uint8)


def _one_pixel(img, y, x):
    out = img.copy()
    out[y, x] = (out[y, x].astype(np.int32) + 97) % 256
    return out


def content_pairs(H, W, seed):
    """(truth, pred) uint8 [9,H,W,3] in the order of CONTENT: the frames AVG_PSNR's temporal border drops are the degenerate ones."""
    rng = np.random.default_rng(seed)
    s = _smooth(rng, H, W)
    noisy = lambda sig: np.clip(np.round(s + rng.normal(0, sig, size=s.shape)), 0, 255).astype(np.uint8)   # noqa: E731
    rnd = lambda: rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)                                      # noqa: E731
    base = rnd()
    pairs = [(base, base.copy()), (s, _one_pixel(s, 0, W - 1)), (rnd(), rnd()), (s, noisy(2)), (s, noisy(6)), (s, noisy(20)),
             (s, _one_pixel(s, 5, 5)), (s, _one_pixel(s, 4, 4)), (np.zeros((H, W, 3), np.uint8), np.full((H, W, 3), 255, np.uint8))]
    return np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])


def _y(u8):
    return metrics.rgb2ycbcr(u8)[..., 0]


def _close(got, want, tol):
    if np.isnan(got) or np.isnan(want):                               # (no frame left inside the temporal border)
        return bool(np.isnan(got) and np.isnan(want))
    return got == want or abs(got - want) <= tol                      # (inf == inf: identical frames)


def per_frame_metrics(truth, pred):
    """pfnl_amd.metrics frame by frame (none of the three depends on the spatial border)."""
    return [{"ssim": metrics.ssim(_y(t), _y(p)), "ssim_valid": metrics.ssim_valid(_y(t), _y(p)), "psnr_y": metrics.psnr_y(t, p)}
            for t, p in zip(truth, pred)]


def check_against_metrics(sums, truth, pred, want, sp_border, label):
    """sums [F,4] of the op against per_frame_metrics and metrics.avg_psnr; every figure is printed before it is asserted."""
    F, H, W, _ = truth.shape
    sc = metrics.sequence_scores(sums, H, W, sp_border=sp_border, t_border=2)
    worst = {"ssim": 0.0, "ssim_valid": 0.0, "psnr_y": 0.0}
    bad = []
    for f in range(F):
        for k, tol in (("ssim", SSIM_TOL), ("ssim_valid", SSIM_TOL), ("psnr_y", PSNR_TOL)):
            got = sc[k][f]
            err = 0.0 if got == want[f][k] else abs(got - want[f][k])
            worst[k] = max(worst[k], err)
            if not _close(got, want[f][k], tol):
                bad.append((label, f, k, got, want[f][k]))
    print("%s sp_border=%d: max |d ssim| %.3g, |d ssim_valid| %.3g, |d psnr_y| %.3g dB" % (
        label, sp_border, worst["ssim"], worst["ssim_valid"], worst["psnr_y"]))
    for tb in (0, 2, 3):
        got = metrics.sequence_scores(sums, H, W, sp_border=sp_border, t_border=tb)["avg_psnr"]
        avg = metrics.avg_psnr(truth, pred, 0.0, 255.0, t_border=tb, sp_border=sp_border)
        print("    avg_psnr t_border=%d: %r (metrics: %r)" % (tb, got, avg))
        if not _close(got, avg, PSNR_TOL):
            bad.append((label, "avg_psnr", tb, got, avg))
    assert not bad, bad
    return sc


def _score(truth, pred, sp_border):
    return ops.score_y(torch.from_numpy(pred).cuda(), torch.from_numpy(truth).cuda(), sp_border).cpu().numpy()


@pytest.mark.parametrize("H,W", SIZES)
def test_score_y_matches_metrics(H, W):
    """Nine kinds of content in ONE call of F = 9, at every size, for the spatial borders the size admits."""
    truth, pred = content_pairs(H, W, seed=H * 1000 + W)
    want = per_frame_metrics(truth, pred)
    for sp in (0, 4, 8):
        if 2 * sp >= min(H, W):
            with pytest.raises(Exception, match="sp_border"):
                _score(truth, pred, sp)
            continue
        sums = _score(truth, pred, sp)
        assert sums.shape == (9, 4) and sums.dtype == np.float64
        sc = check_against_metrics(sums, truth, pred, want, sp, "%dx%d" % (H, W))
        assert sc["psnr_y"][0] == float("inf") and abs(sc["ssim"][0] - 1.0) < 1e-12 and abs(sc["ssim_valid"][0] - 1.0) < 1e-12
        assert sums[0, 0] == 0.0 and sums[0, 1] == 0.0
        if sp == 0:
            assert np.array_equal(sums[:, 0], sums[:, 1])               # no border: the crop is the frame
        else:
            assert sums[1, 0] > 0.0 and sums[1, 1] == 0.0              # the corner pixel lies outside every crop
        # the single pixel at (5, 5) lies inside [4:-4] and outside [8:-8]; (4, 4) is the first pixel of [4:-4]
        assert (sums[6, 1] > 0.0) == (sp <= 5) and (sums[7, 1] > 0.0) == (sp <= 4)
        # a frame scored alone has the bits it has inside the batch
        for f in (2, 8):
            assert np.array_equal(_score(truth[f:f + 1], pred[f:f + 1], sp), sums[f:f + 1])


def test_score_y_is_repeatable_and_stream_ordered():
    """Two calls return identical bits; the op runs on the caller's (non-default) stream."""
    truth, pred = content_pairs(144, 180, seed=7)
    t, p = torch.from_numpy(truth).cuda(), torch.from_numpy(pred).cuda()
    a = ops.score_y(p, t, 8)
    b = ops.score_y(p, t, 8)
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        p2 = p.clone()                                                # produced on the side stream: the op must run behind it
        p2[2] = t[2]
        c = ops.score_y(p2, t, 8)
    side.synchronize()
    c = c.cpu().numpy()
    a = a.cpu().numpy()
    assert c[2, 0] == 0.0 and np.array_equal(np.delete(c, 2, 0), np.delete(a, 2, 0))
    with pytest.raises(TypeError):
        ops.score_y(p.float(), t, 8)
    with pytest.raises(ValueError):
        ops.score_y(p[:, :100].contiguous(), t, 8)


# ---- the harness ------------------------------------------------------------------------------------------------------------

def _sequence(root, name, hr_u8):
    from PIL import Image
    seq = root / name
    (seq / "truth").mkdir(parents=True)
    for i, im in enumerate(hr_u8):
        Image.fromarray(im).save(seq / "truth" / f"{i:04d}.png")
    return seq


def _model(tmp_path, weights=None):
    from model.pfnl import PFNL
    m = PFNL()
    m.num_block = 1
    m.save_dir = str(tmp_path / "none")
    m.set_weights(weights if weights is not None else synth.synthetic_weights(PFNLGeometry(num_block=1), seed=0))
    return m


def _pngs(d):
    from PIL import Image
    return np.stack([np.asarray(Image.open(p)) for p in sorted(d.glob("*.png"))])


def check_scores_of_pngs(sc, sr, truth):
    """The dict score_video_truth returned against metrics applied to the PNGs read back and the truth PNGs."""
    F = truth.shape[0]
    assert len(sc["psnr_y"]) == len(sc["ssim"]) == len(sc["ssim_valid"]) == F
    want = {"psnr_y": [metrics.psnr_y(truth[f], sr[f]) for f in range(F)],
            "ssim": [metrics.ssim(_y(truth[f]), _y(sr[f])) for f in range(F)],
            "ssim_valid": [metrics.ssim_valid(_y(truth[f]), _y(sr[f])) for f in range(F)]}
    for k, tol in (("psnr_y", PSNR_TOL), ("ssim", SSIM_TOL), ("ssim_valid", SSIM_TOL)):
        err = max(0.0 if g == w else abs(g - w) for g, w in zip(sc[k], want[k]))
        print("harness %dx%d: max |d %s| = %.3g" % (truth.shape[1], truth.shape[2], k, err))
        assert err <= tol, (k, sc[k], want[k])
        assert _close(sc[k + "_mean"], float(np.mean(want[k])), tol)
    avg = metrics.avg_psnr(truth, sr, 0.0, 255.0)
    print("    avg_psnr %r (metrics: %r)" % (sc["avg_psnr"], avg))
    assert _close(sc["avg_psnr"], avg, PSNR_TOL)


@pytest.mark.parametrize("H,W,part", [(64, 96, 4), (576, 720, 50)])
def test_video_truth_scores_what_it_writes(tmp_path, monkeypatch, capsys, H, W, part):
    """9 random HR frames (64 x 96 with part 4: batches of 3; the Vid4 geometry 576 x 720 with one window per forward): score_video_truth
    writes the bytes test_video_truth writes and returns the scores of those PNGs against the truth PNGs; test_video_truth returns None."""
    rng = np.random.default_rng(H + W)
    hr = rng.integers(0, 256, size=(9, H, W, 3), dtype=np.uint8)
    seq = _sequence(tmp_path, "calendar", hr)
    m = _model(tmp_path)
    assert m.test_video_truth(str(seq), name="plain", part=part) is None
    capsys.readouterr()
    sc = m.score_video_truth(str(seq), name="scored", part=part)
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("calendar: PSNR_Y ")]
    assert line == ['calendar: PSNR_Y {:.4f} dB, AVG_PSNR {:.4f} dB, SSIM {:.6f}'.format(sc["psnr_y_mean"], sc["avg_psnr"], sc["ssim_mean"])]
    names = sorted(p.name for p in (seq / "plain").glob("*.png"))
    assert names == ["%04d.png" % i for i in range(9)]
    for n in names:
        assert (seq / "plain" / n).read_bytes() == (seq / "scored" / n).read_bytes()
    check_scores_of_pngs(sc, _pngs(seq / "scored"), hr)
    if part == 4:                                                     # two forwards in flight: each lane scores its own batches
        monkeypatch.setenv("PFNL_HARNESS_INFLIGHT", "2")
        sc2 = m.score_video_truth(str(seq), name="scored2", part=part)
        assert sc2 == sc
        for n in names:
            assert (seq / "plain" / n).read_bytes() == (seq / "scored2" / n).read_bytes()


def test_testvideos_scores_every_sequence(tmp_path, capsys):
    """score_videos: one entry per sequence directory.  The second sequence's HR size is no multiple of the scale: the SR
    frame (4 * ceil(H / 4)) is larger, the common top-left region is scored and the printed line says so."""
    rng = np.random.default_rng(5)
    hrs = {"city": rng.integers(0, 256, size=(3, 32, 48, 3), dtype=np.uint8),
           "walk": rng.integers(0, 256, size=(5, 46, 54, 3), dtype=np.uint8)}
    for name, hr in hrs.items():
        _sequence(tmp_path, name, hr)
    m = _model(tmp_path)
    assert m.testvideos(str(tmp_path), name="plain") is None
    capsys.readouterr()
    got = m.score_videos(str(tmp_path), name="pfnl")
    out = capsys.readouterr().out
    assert sorted(got) == ["city", "walk"]
    assert "score: HR 46 x 54 and SR 48 x 56 are compared over their common top-left 46 x 54" in out
    assert sum(ln.startswith(("city: PSNR_Y", "walk: PSNR_Y")) for ln in out.splitlines()) == 2
    for name, hr in hrs.items():
        sr = _pngs(tmp_path / name / "pfnl")
        assert np.array_equal(sr, _pngs(tmp_path / name / "plain"))
        assert sr.shape[1:3] == (-(-hr.shape[1] // 4) * 4, -(-hr.shape[2] // 4) * 4)
        check_scores_of_pngs(got[name], sr[:, :hr.shape[1], :hr.shape[2]], hr)
    assert np.isnan(got["city"]["avg_psnr"])                         # 3 frames: AVG_PSNR's temporal border leaves none


def test_scores_follow_the_range_flag_recomputation(tmp_path):
    """The scaled weights of test_harness_reruns_out_of_range_batches (conv0 x 4e5, convmerge2 x 1e-6): the first batch leaves binary16's
    range, it and the batch behind it are recomputed on the strict kernels - and scored AGAIN: the scores are those of the PNGs that
    were written (those of a strict engine), not of the frames the f16 pipe produced first."""
    from pfnl_amd import model as M
    from pfnl_amd.engine import PFNLEngine
    rng = np.random.default_rng(21)
    hr = rng.integers(0, 256, size=(7, 48, 80, 3), dtype=np.uint8)
    seq = _sequence(tmp_path, "seqR", hr)
    geom = PFNLGeometry(num_block=1)
    w = synth.synthetic_weights(geom, seed=1)
    w["nlvsr/conv0/kernel"] = (w["nlvsr/conv0/kernel"] * 4e5).astype(np.float32)
    w["nlvsr/convmerge2/kernel"] = (w["nlvsr/convmerge2/kernel"] * 1e-6).astype(np.float32)
    m = _model(tmp_path, w)
    sc = m.score_video_truth(str(seq), name="out", part=3)  # 7 frames, part 3 -> batches of 3, 3, 1
    got = _pngs(seq / "out")
    lrs = ops.blur_decimate(torch.from_numpy((hr / 255.).astype(np.float32)).cuda(), 4).cpu().numpy()
    eng = PFNLEngine(geom, device=0)
    eng.load_weights(w)
    eng.set_option("strict_fp32", "on")
    sr = eng.forward(np.ascontiguousarray(M.sliding_windows(lrs, 7)))
    eng.close()
    assert np.isfinite(sr).all() and np.array_equal(got, M.quantise(sr[:, 0]))   # the recomputed frames are what was written
    check_scores_of_pngs(sc, got, hr)
    assert m._get_engine().range_flagged() is False
    y = m.forward(lrs[None, :7])                                      # the engine is back on its default kernels afterwards
    assert np.isfinite(y).all() and m._get_engine().range_reruns() == 1
