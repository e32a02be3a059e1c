"""Times the two format kernels of the streaming session (pfnl_amd/csrc/yuv.hip) against the floor they are judged by - a device-to-device
hipMemcpyAsync that moves the same number of bytes (read plus written) - and one streamed sequence with NV12 frames in and out against the
same sequence in RGB.  HIP events around `inner` back-to-back launches, the median of `repeats` such groups.

    python tools/yuv_timing.py [--repeats 30] [--inner 20] [--frames 32] [--num-block 20]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--num-block", type=int, default=20)
    a = ap.parse_args()
    import torch
    from pfnl_amd import ops, synth, yuv
    from pfnl_amd.engine import PFNLEngine
    from pfnl_amd.spec import PFNLGeometry
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    stream = torch.cuda.current_stream()

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        us = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(a.inner):
                fn()
            e1.record(stream)
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / a.inner)
        return statistics.median(us), min(us)

    rng = np.random.default_rng(0)
    rows = []
    for name, n, H, W in (("yuv420_to_rgb_u8", 1, 270, 480), ("rgb_to_yuv420_u8", 4, 1080, 1920)):
        yb, rb = n * H * W * 3 // 2, n * H * W * 3
        moved = yb + rb                                                          # bytes read plus bytes written, either direction
        a_buf = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
        b_buf = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
        copy = lambda: hip.hipMemcpyAsync(b_buf.data_ptr(), a_buf.data_ptr(), moved // 2, 3, stream.cuda_stream)   # noqa: E731  (reads and writes `moved` in all)
        for fmt in ("nv12", "i420"):
            if name == "yuv420_to_rgb_u8":
                src = torch.from_numpy(rng.integers(0, 256, (n, H * 3 // 2, W), np.uint8)).cuda()
                dst = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
                fn = lambda: ops.yuv420_to_rgb(src, fmt, H, W, out=dst)         # noqa: E731
            else:
                src = torch.from_numpy(rng.integers(0, 256, (n, H, W, 3), np.uint8)).cuda()
                dst = torch.empty((n, H * 3 // 2, W), dtype=torch.uint8, device="cuda")
                fn = lambda: ops.rgb_to_yuv420(src, fmt, out=dst)               # noqa: E731
            k_med, k_min = timed(fn)
            c_med, c_min = timed(copy)
            rows.append({"kernel": name, "fmt": fmt, "n": n, "H": H, "W": W, "bytes_moved": moved, "kernel_us": round(k_med, 2),
                         "kernel_us_min": round(k_min, 2), "copy_us": round(c_med, 2), "copy_us_min": round(c_min, 2),
                         "kernel_GBps": round(moved / k_med / 1e3, 1), "ratio_to_copy": round(k_med / c_med, 2)})
            print(json.dumps(rows[-1]), flush=True)

    H, W, batch = 270, 480, 4
    geom = PFNLGeometry(num_block=a.num_block)
    eng = PFNLEngine(geom, device=0)
    eng.load_weights(synth.synthetic_weights(geom, seed=0))
    rgb = list(rng.integers(0, 256, (a.frames, H, W, 3), np.uint8))
    nv12 = [yuv.from_rgb(f, "nv12") for f in rgb]
    for label, frames, kw in (("rgb24", rgb, {}), ("nv12", nv12, {"pixel_format": "nv12"})):
        best = None
        for _ in range(3):
            with eng.open_stream(H, W, batch, **kw) as vs:
                t0 = time.perf_counter()
                count = 0
                for f in frames:
                    count += len(vs.push(f))
                count += len(vs.end())
                dt = time.perf_counter() - t0
            assert count == a.frames
            best = dt if best is None else min(best, dt)
        print(json.dumps({"session": label, "H": H, "W": W, "batch": batch, "num_block": a.num_block, "frames": a.frames,
                          "seconds_best_of_3": round(best, 4), "fps": round(a.frames / best, 2)}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
