"""What scoring on the device costs (DESIGN.md "Scores on the device"):
  op       device time of pfnl_op_score_y per 576x720 and per 2160x3840 frame (F = 8, HIP events around enough launches to fill
           half a second, after warm-up);
  host     what it replaces: metrics.ssim + metrics.psnr_y per 576x720 frame on this machine's CPU;
  harness  test_video_truth against score_video_truth on a 41-frame sequence of 576x720 HR frames (144x180 LR, the Vid4 geometry,
           one window per forward), alternating, three runs each: wall time and the device time per frame the harness prints.
usage: python tools/score_timing.py [op] [host] [harness]        (default: all three)"""
import contextlib
import io
import os
import re
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402


def time_op():
    import torch
    from pfnl_amd import ops
    for H, W in ((576, 720), (2160, 3840)):
        g = torch.Generator(device="cuda").manual_seed(H)
        truth = torch.randint(0, 256, (8, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
        pred = (truth.int() + torch.randint(-6, 7, truth.shape, device="cuda", generator=g)).clamp(0, 255).to(torch.uint8)
        for _ in range(3):
            ops.score_y(pred, truth, 8)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            ops.score_y(pred, truth, 8)
        torch.cuda.synchronize()
        n = max(10, int(0.5 / ((time.perf_counter() - t0) / 10)) + 1)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            ops.score_y(pred, truth, 8)
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b) / n
        print("op %dx%d: %d launches of F=8, %.3f ms per launch, %.2f us per frame, %.1f GB/s of frame bytes" % (
            H, W, n, ms, ms * 1e3 / 8, 8 * H * W * 6 / (ms * 1e-3) / 1e9), flush=True)


def time_host():
    from pfnl_amd import metrics
    rng = np.random.default_rng(0)
    a = rng.integers(0, 256, size=(576, 720, 3), dtype=np.uint8)
    b = np.clip(a + rng.integers(-6, 7, size=a.shape), 0, 255).astype(np.uint8)
    ts = []
    for _ in range(4):
        t0 = time.perf_counter()
        metrics.ssim(metrics.rgb2ycbcr(a)[..., 0], metrics.rgb2ycbcr(b)[..., 0])
        metrics.psnr_y(a, b)
        ts.append(time.perf_counter() - t0)
    print("host 576x720: metrics.ssim + metrics.psnr_y %.1f ms per frame (best of %d after one warm-up; %s)" % (
        min(ts[1:]) * 1e3, len(ts) - 1, ", ".join("%.1f" % (t * 1e3) for t in ts[1:])), flush=True)


def time_harness():
    from PIL import Image
    from model.pfnl import PFNL
    from pfnl_amd import synth
    from pfnl_amd.spec import PFNLGeometry
    d = tempfile.mkdtemp()
    seq = os.path.join(d, "seq")
    os.makedirs(os.path.join(seq, "truth"))
    rng = np.random.default_rng(0)
    base = rng.integers(0, 256, size=(576 + 48, 720 + 96, 3), dtype=np.uint8)
    frames = 41
    for i in range(frames):
        Image.fromarray(base[i:i + 576, 2 * i:2 * i + 720]).save(os.path.join(seq, "truth", "%04d.png" % i))
    m = PFNL()
    m.save_dir = os.path.join(d, "none")
    m.set_weights(synth.synthetic_weights(PFNLGeometry(), seed=0))

    def run(fn, name):
        buf = io.StringIO()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(buf):
            fn(seq, name=name, part=50)
        wall = time.perf_counter() - t0
        return wall, float(re.search(r"and ([0-9.eE+-]+) s in average", buf.getvalue()).group(1))

    run(m.test_video_truth, "warm0")
    run(m.score_video_truth, "warm1")
    res = {"plain": [], "scored": []}
    for i in range(3):
        res["plain"].append(run(m.test_video_truth, "plain%d" % i))
        res["scored"].append(run(m.score_video_truth, "scored%d" % i))
    for k, v in res.items():
        print("harness %s: wall per frame %s ms, device time per frame %s ms" % (
            k, ", ".join("%.3f" % (w / frames * 1e3) for w, _ in v), ", ".join("%.3f" % (t * 1e3) for _, t in v)), flush=True)
    med = lambda k, j: float(np.median([r[j] for r in res[k]]))   # noqa: E731
    print("harness: scoring adds %.3f ms of wall and %.3f ms of device time per frame (medians) beside %.3f ms per frame of the "
          "unscored batches" % ((med("scored", 0) - med("plain", 0)) / frames * 1e3, (med("scored", 1) - med("plain", 1)) * 1e3,
                                med("plain", 1) * 1e3), flush=True)


if __name__ == "__main__":
    what = sys.argv[1:] or ["op", "host", "harness"]
    for w in what:
        {"op": time_op, "host": time_host, "harness": time_harness}[w]()
