"""What the chroma sitings cost (DESIGN.md "Chroma siting"; include/pfnl_hip.h SITING).  Workloads: the decode (NV12 / I420 -> RGB) and the
encode (RGB -> NV12 / I420) of --frames frames at each of --sizes, device tensors, HIP events, everything in one process, the cases
alternating over --rounds rounds after a warm-up of every case.  Per size, direction and format: the median milliseconds of one call per
siting, its spread over the rounds (max - min) / median, and the GB/s of the bytes it reads and writes.
  --plain     time the hooks without a siting argument (pfnl_op_yuv420_to_rgb_u8, pfnl_op_rgb_to_yuv420_u8) and nothing else
  --lib PATH  another build of the library, e.g. one of the commit before the sitings: with --plain its left-sited kernels, in the same
              session on the same device, are what the "left" rows compare against
usage: python tools/bench_siting.py [--rounds 7] [--reps 20] [--frames 8] [--sizes 270x480,1080x1920] [--plain] [--lib PATH] [--out result.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FMT = {"nv12": 1, "i420": 2}
SITINGS = ("left", "center", "topleft")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20, help="calls inside one timed window")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--sizes", default="270x480,1080x1920")
    ap.add_argument("--plain", action="store_true")
    ap.add_argument("--lib", default=os.path.join(ROOT, "pfnl_amd", "lib", "libpfnl_hip.so"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    lib = C.CDLL(a.lib, mode=C.RTLD_GLOBAL)                                      # (raw: a build without the sited hooks loads as well)
    vp, i = C.c_void_p, C.c_int
    lib.pfnl_last_error.restype = C.c_char_p
    for name in ("pfnl_op_yuv420_to_rgb_u8", "pfnl_op_rgb_to_yuv420_u8"):
        getattr(lib, name).argtypes = [vp, i, i, i, i, i, i, vp, vp]
    if not a.plain:
        for name in ("pfnl_op_yuv420_to_rgb_u8_sited", "pfnl_op_rgb_to_yuv420_u8_sited"):
            getattr(lib, name).argtypes = [vp, i, i, i, i, i, i, vp, i, vp]
    res = {"device": torch.cuda.get_device_name(0), "lib": os.path.relpath(a.lib, ROOT), "plain": a.plain, "rounds": a.rounds, "reps": a.reps,
           "frames": a.frames, "cases": []}
    stream = vp(torch.cuda.current_stream().cuda_stream or None)

    def call(decode, fmt, siting, src, dst, n, H, W):
        name = "pfnl_op_yuv420_to_rgb_u8" if decode else "pfnl_op_rgb_to_yuv420_u8"
        if a.plain:
            st = getattr(lib, name)(vp(src.data_ptr()), FMT[fmt], 1, 0, n, H, W, vp(dst.data_ptr()), stream)
        else:
            st = getattr(lib, name + "_sited")(vp(src.data_ptr()), FMT[fmt], 1, 0, n, H, W, vp(dst.data_ptr()), SITINGS.index(siting), stream)
        if st:
            raise RuntimeError(lib.pfnl_last_error().decode())

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
        yuv = torch.randint(0, 256, (n, H * 3 // 2, W), dtype=torch.uint8, device="cuda", generator=g)
        rgb = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
        yuv_out, rgb_out = torch.empty_like(yuv), torch.empty_like(rgb)
        work = {}
        for fmt in FMT:
            for siting in (("left",) if a.plain else SITINGS):
                work[("decode", fmt, siting)] = lambda fmt=fmt, siting=siting: call(True, fmt, siting, yuv, rgb_out, n, H, W)
                work[("encode", fmt, siting)] = lambda fmt=fmt, siting=siting: call(False, fmt, siting, rgb, yuv_out, n, H, W)
        moved = yuv.numel() + rgb.numel()                                        # either direction reads one and writes the other
        for (direction, fmt, siting), ms in timed(work).items():
            med = statistics.median(ms)
            case = {"size": f"{n}x{H}x{W}", "direction": direction, "fmt": fmt, "siting": siting, "ms": med, "spread": (max(ms) - min(ms)) / med,
                    "GBps": moved / (med * 1e-3) / 1e9}
            res["cases"].append(case)
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
