"""What the colour stage 0 costs (include/pfnl_hip.h COLOUR).  Workload: --frames SR frames of --size as fp32 through
pfnl_op_quantise_colour_u8 / _u10 (bt601-525 -> bt709), through the plain pfnl_op_quantise_u8 / _u10, and a device-to-device copy that
moves the same bytes (half of what the kernel reads and writes, read once and written once), all on device tensors in one process, timed
with HIP events over --reps calls, the cases alternating over --rounds rounds after a warm-up of every case.  The table reads are gathers
by value, so two pictures are timed: uniform noise (every lane another table entry) and a smooth ramp (neighbours share entries).  Per
case: the median milliseconds of one call, its spread over the rounds (max - min) / median, the GB/s of the bytes it reads and writes, and
its time over the plain quantise's and the copy's of the same depth.
usage: python tools/bench_colour.py [--rounds 7] [--reps 50] [--frames 8] [--size 1080x1920] [--out result.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50, help="calls inside one timed window")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", default="1080x1920")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from pfnl_amd import _capi
    lib = _capi.load_library()
    H, W = (int(v) for v in a.size.split("x"))
    pixels = a.frames * H * W
    if pixels % 4:
        raise SystemExit("frames * H * W must be a multiple of 4")
    vp = C.c_void_p
    stream = vp(torch.cuda.current_stream().cuda_stream or None)
    g = torch.Generator(device="cuda").manual_seed(1)
    pictures = {"noise": torch.rand((pixels, 3), dtype=torch.float32, device="cuda", generator=g),
                "ramp": (torch.arange(pixels * 3, dtype=torch.float32, device="cuda") / float(pixels * 3)).view(pixels, 3)}
    outs = {8: torch.empty((pixels, 3), dtype=torch.uint8, device="cuda"), 10: torch.empty((pixels, 3), dtype=torch.uint16, device="cuda")}
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "frames": a.frames, "size": a.size, "cases": []}

    def check(st):
        if st:
            raise RuntimeError(lib.pfnl_last_error().decode())

    work, moved = {}, {}
    for bits, plain, hook in ((8, lib.pfnl_op_quantise_u8, lib.pfnl_op_quantise_colour_u8), (10, lib.pfnl_op_quantise_u10, lib.pfnl_op_quantise_colour_u10)):
        out = outs[bits]
        nbytes = pixels * 3 * 4 + out.numel() * out.element_size()
        half = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
        half_out = torch.empty_like(half)
        work[("copy", bits, "-")] = lambda half=half, half_out=half_out: half_out.copy_(half)
        moved[("copy", bits, "-")] = 2 * half.numel()
        for name, x in pictures.items():
            work[("quantise", bits, name)] = lambda x=x, out=out, plain=plain: check(plain(vp(x.data_ptr()), vp(out.data_ptr()), x.numel(), stream))
            work[("colour", bits, name)] = lambda x=x, out=out, hook=hook: check(hook(vp(x.data_ptr()), vp(out.data_ptr()), pixels, 1, 0, stream))
            moved[("quantise", bits, name)] = moved[("colour", bits, name)] = nbytes

    for f in work.values():                                                      # every case once, twice
        f()
        f()
    torch.cuda.synchronize()
    ms = {k: [] for k in work}
    for _ in range(a.rounds):
        for key, f in work.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            ms[key].append(e0.elapsed_time(e1) / a.reps)
    med = {k: statistics.median(v) for k, v in ms.items()}
    for (kind, bits, picture), v in ms.items():
        case = {"kind": kind, "bits": bits, "picture": picture, "ms": med[(kind, bits, picture)], "spread": (max(v) - min(v)) / med[(kind, bits, picture)],
                "GBps": moved[(kind, bits, picture)] / (med[(kind, bits, picture)] * 1e-3) / 1e9}
        if kind == "colour":
            case["over_quantise"] = case["ms"] / med[("quantise", bits, picture)]
            case["over_copy"] = case["ms"] / med[("copy", bits, "-")]
        if kind == "quantise":
            case["over_copy"] = case["ms"] / med[("copy", bits, "-")]
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
