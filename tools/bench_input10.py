"""What 10-bit input costs (include/pfnl_hip.h 10 BITS IN).  Workloads: the decode of --frames frames (P010 / I010
-> RGB10 at the three sitings, next to NV12 / I420 -> RGB24) and the gather of one batch of --frames windows of T = 7 from a ring of uint16
samples, next to the one from a ring of uint8, at each of --sizes; device tensors, HIP events, everything in one process, the cases
alternating over --rounds rounds after a warm-up of every case.  Per case: the median milliseconds of one call, its spread over the rounds
(max - min) / median, the GB/s of the bytes it reads and writes, and for a 10-bit case the ratio of its median to its 8-bit twin's.
usage: python tools/bench_input10.py [--rounds 7] [--reps 20] [--frames 8] [--sizes 270x480,1080x1920] [--out result.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SITINGS = ("left", "center", "topleft")
TWIN = {"p010": "nv12", "i010": "i420"}
T = 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20, help="calls inside one timed window")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--sizes", default="270x480,1080x1920")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from pfnl_amd import ops
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "frames": a.frames, "cases": []}

    def timed(work):
        for f in work.values():                                                  # every case once, twice
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
        return ms

    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        n = a.frames
        g = torch.Generator(device="cuda").manual_seed(1)
        yuv8 = torch.randint(0, 256, (n, H * 3 // 2, W), dtype=torch.uint8, device="cuda", generator=g)
        i010 = torch.randint(0, 1024, (n, H * 3 // 2, W), dtype=torch.int16, device="cuda", generator=g)
        yuv10 = {"i010": i010.view(torch.uint16), "p010": (i010 << 6).view(torch.uint16)}
        rgb8 = torch.empty((n, H, W, 3), dtype=torch.uint8, device="cuda")
        rgb10 = torch.empty((n, H, W, 3), dtype=torch.uint16, device="cuda")
        cap = n + T - 1                                                          # the frames one batch of n windows names
        ring8 = torch.randint(0, 256, (cap, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
        ring10 = torch.randint(0, 1024, (cap, H, W, 3), dtype=torch.int16, device="cuda", generator=g).view(torch.uint16)
        work, moved = {}, {}
        for siting in SITINGS:
            for fmt, twin in TWIN.items():
                work[("decode", twin, siting)] = lambda twin=twin, siting=siting: ops.yuv420_to_rgb(yuv8, twin, H, W, out=rgb8, siting=siting)
                work[("decode", fmt, siting)] = lambda fmt=fmt, siting=siting: ops.yuv420_to_rgb10(yuv10[fmt], fmt, H, W, out=rgb10, siting=siting)
                moved[("decode", twin, siting)] = yuv8.numel() + rgb8.numel()
                moved[("decode", fmt, siting)] = 2 * (i010.numel() + rgb10.numel())
        work[("gather", "u8", "-")] = lambda: ops.gather_windows_u8(ring8, cap - 1, T // 2, n, T)
        work[("gather", "u10", "-")] = lambda: ops.gather_windows_u10(ring10, cap - 1, T // 2, n, T)
        win = n * T * H * W * 3                                                  # samples read (each from cache or memory) and floats written
        moved[("gather", "u8", "-")] = win * (1 + 4)
        moved[("gather", "u10", "-")] = win * (2 + 4)
        med = {}
        for key, ms in timed(work).items():
            med[key] = statistics.median(ms)
            case = {"size": f"{n}x{H}x{W}", "op": key[0], "fmt": key[1], "siting": key[2], "ms": med[key], "spread": (max(ms) - min(ms)) / med[key],
                    "GBps": moved[key] / (med[key] * 1e-3) / 1e9}
            res["cases"].append(case)
        for case in res["cases"]:
            twin = {"p010": "nv12", "i010": "i420", "u10": "u8"}.get(case["fmt"])
            if twin and case["size"] == f"{n}x{H}x{W}":
                case["ratio_to_8bit"] = case["ms"] / med[(case["op"], twin, case["siting"])]
            if case["size"] == f"{n}x{H}x{W}":
                print(json.dumps(case), flush=True)
    torch.cuda.synchronize()
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    assert all(c["ms"] > 0 for c in res["cases"])


if __name__ == "__main__":
    main()
