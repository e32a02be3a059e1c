"""What 4:2:2 and 4:4:4 cost next to 4:2:0 (include/pfnl_hip.h CHROMA FORMAT).  Workloads: the decode and the encode of
--frames frames of --size in both layouts (nv12 | i420) at both depths, at 4:2:2 (co-sited and midway) and 4:4:4, and THE 4:2:0 KERNEL OF THE
SAME LAYOUT AND DEPTH IN THE SAME RUN as the yardstick; device tensors, HIP events, everything in one process, the cases alternating over
--rounds rounds after a warm-up of every case.  Per case: the median milliseconds of one call, its spread over the rounds (max - min) /
median, the TB/s of the bytes it reads and writes, the ratio of its median to its 4:2:0 twin's and the ratio of their bytes (the byte
model: 4.5, 5 and 6 samples moved per pixel), and whether the first exceeds the second by more than the twin's spread.
usage: python tools/bench_chroma.py [--rounds 7] [--reps 1000] [--frames 8] [--size 1080x1920] [--out result.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = (("420", "left"), ("422", "left"), ("422", "center"), ("444", "left"))
SAMPLES = {"420": 1.5, "422": 2.0, "444": 3.0}                                   # of a YUV frame, per pixel; the RGB side has 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=1000, help="calls inside one timed window")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", default="1080x1920")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from pfnl_amd import ops
    H, W = (int(v) for v in a.size.split("x"))
    n = a.frames
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "size": f"{n}x{H}x{W}", "cases": []}
    g = torch.Generator(device="cuda").manual_seed(1)
    work, moved = {}, {}
    for bits in (8, 10):
        dt, sz = (torch.uint8, 1) if bits == 8 else (torch.uint16, 2)
        layouts = ("nv12", "i420") if bits == 8 else ("p010", "i010")
        dec, enc = (ops.yuv_to_rgb, ops.rgb_to_yuv) if bits == 8 else (ops.yuv_to_rgb_u10, ops.rgb_to_yuv_u10)
        rgb_in = torch.randint(0, 1 << bits, (n, H, W, 3), dtype=torch.int16, device="cuda", generator=g).to(torch.uint8) if bits == 8 else \
            torch.randint(0, 1024, (n, H, W, 3), dtype=torch.int16, device="cuda", generator=g).view(torch.uint16)
        rgb_out = torch.empty((n, H, W, 3), dtype=dt, device="cuda")
        for chroma, siting in CASES:
            rows = int(H * SAMPLES[chroma])
            for fmt in layouts:
                if bits == 8:
                    src = torch.randint(0, 256, (n, rows, W), dtype=torch.int16, device="cuda", generator=g).to(torch.uint8)
                else:
                    v = torch.randint(0, 1024, (n, rows, W), dtype=torch.int16, device="cuda", generator=g)
                    src = (v << 6 if fmt == "p010" else v).view(torch.uint16)
                dst = torch.empty((n, rows, W), dtype=dt, device="cuda")
                work[("decode", bits, fmt, chroma, siting)] = lambda dec=dec, src=src, fmt=fmt, chroma=chroma, siting=siting, out=rgb_out: \
                    dec(src, fmt, H, W, chroma=chroma, siting=siting, out=out)
                work[("encode", bits, fmt, chroma, siting)] = lambda enc=enc, x=rgb_in, fmt=fmt, chroma=chroma, siting=siting, out=dst: \
                    enc(x, fmt, chroma=chroma, siting=siting, out=out)
                for op in ("decode", "encode"):
                    moved[(op, bits, fmt, chroma, siting)] = int(n * H * W * (SAMPLES[chroma] + 3.0) * sz)

    for f in work.values():                                                      # every case once, twice
        f()
        f()
    torch.cuda.synchronize()
    ms = {k: [] for k in work}
    for _ in range(a.rounds):
        for name, f in work.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.reps)
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}
    for key in work:
        op, bits, fmt, chroma, siting = key
        twin = (op, bits, fmt, "420", "left")
        case = {"op": op, "bits": bits, "fmt": fmt, "chroma": chroma, "siting": siting, "ms": med[key], "spread": spread[key],
                "TBps": moved[key] / (med[key] * 1e-3) / 1e12, "ratio_to_420": med[key] / med[twin], "byte_ratio": moved[key] / moved[twin],
                "spread_of_420": spread[twin]}
        case["above_byte_model"] = case["ratio_to_420"] > case["byte_ratio"] * (1.0 + spread[twin])
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    assert all(c["ms"] > 0 for c in res["cases"])


if __name__ == "__main__":
    main()
