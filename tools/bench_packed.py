"""What a packed format costs next to the planar kernel that moves the most similar bytes (include/pfnl_hip.h PACKED
FORMATS).  Workloads: the decode and the encode of --frames frames of --size in every packing (pfnl_amd/packed.py PACKINGS), and IN THE SAME
RUN the yardstick of each: for a 4:2:2 packing the planar 4:2:2 kernel of its depth (I422 through ops.yuv_to_rgb / rgb_to_yuv, yuv422p10le
through the _u10 pair), for an RGB packing a device-to-device copy of the bytes the kernel reads and writes (half of them each way).  Device
tensors, HIP events, everything in one process, the cases alternating over --rounds rounds after a warm-up of every case.  Per case: the
median microseconds of one call, its spread over the rounds (max - min) / median, the TB/s of the bytes it reads and writes, the ratio of
its median to its yardstick's and the ratio of their bytes.
usage: python tools/bench_packed.py [--rounds 7] [--reps 300] [--frames 8] [--size 1080x1920] [--out result.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=300, help="calls inside one timed window")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", default="1080x1920", help="HxW; W a multiple of 6 for v210 (1920 is)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from pfnl_amd import ops
    from pfnl_amd import packed as P
    H, W = (int(v) for v in a.size.split("x"))
    n = a.frames
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "size": f"{n}x{H}x{W}", "cases": []}
    g = torch.Generator(device="cuda").manual_seed(1)
    rand = lambda shape, top: torch.randint(0, top, shape, dtype=torch.int16, device="cuda", generator=g)   # noqa: E731
    work, moved, twin = {}, {}, {}
    for bits in (8, 10):
        dt, sz = (torch.uint8, 1) if bits == 8 else (torch.uint16, 2)
        rgb_in = rand((n, H, W, 3), 1 << bits).to(torch.uint8) if bits == 8 else rand((n, H, W, 3), 1024).view(torch.uint16)
        rgb_out = torch.empty((n, H, W, 3), dtype=dt, device="cuda")
        rgb_bytes = n * H * W * 3 * sz
        # the planar 4:2:2 twins of this depth
        fmt = "i420" if bits == 8 else "i010"
        dec, enc = (ops.yuv_to_rgb, ops.rgb_to_yuv) if bits == 8 else (ops.yuv_to_rgb_u10, ops.rgb_to_yuv_u10)
        src = rand((n, 2 * H, W), 1 << bits).to(torch.uint8) if bits == 8 else rand((n, 2 * H, W), 1024).view(torch.uint16)
        dst = torch.empty((n, 2 * H, W), dtype=dt, device="cuda")
        for siting in ("left", "center"):
            work[("decode", "planar422", bits, siting)] = lambda dec=dec, src=src, fmt=fmt, siting=siting, out=rgb_out: \
                dec(src, fmt, H, W, chroma="422", siting=siting, out=out)
            work[("encode", "planar422", bits, siting)] = lambda enc=enc, fmt=fmt, x=rgb_in, siting=siting, out=dst: \
                enc(x, fmt, chroma="422", siting=siting, out=out)
            for op in ("decode", "encode"):
                moved[(op, "planar422", bits, siting)] = n * H * W * 2 * sz + rgb_bytes
        for name in P.PACKINGS[1:]:
            if P.bits(name) != bits:
                continue
            fb = P.frame_bytes(name, H, W)
            packed_in = torch.randint(0, 256, (n, fb), dtype=torch.int16, device="cuda", generator=g).to(torch.uint8)
            packed_out = torch.zeros((n, fb), dtype=torch.uint8, device="cuda")
            for siting in (("left", "center") if P.is_yuv(name) else ("left",)):
                work[("decode", name, bits, siting)] = lambda name=name, x=packed_in, siting=siting, out=rgb_out: \
                    ops.packed_to_rgb(x, name, H, W, siting=siting, out=out)
                work[("encode", name, bits, siting)] = lambda name=name, x=rgb_in, siting=siting, out=packed_out: \
                    ops.rgb_to_packed(x, name, siting=siting, out=out)
                for op in ("decode", "encode"):
                    moved[(op, name, bits, siting)] = n * H * P.row_bytes(name, W) + rgb_bytes
                    twin[(op, name, bits, siting)] = (op, "planar422", bits, siting) if P.is_yuv(name) else ("copy", name, bits, "left")
            if not P.is_yuv(name):                                               # the copy that moves the kernel's bytes: half of them, read and written
                half = (n * H * P.row_bytes(name, W) + rgb_bytes) // 2
                a_, b_ = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
                work[("copy", name, bits, "left")] = lambda a_=a_, b_=b_: b_.copy_(a_)
                moved[("copy", name, bits, "left")] = 2 * half

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
    spread = {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}
    for key in work:
        op, name, bits, siting = key
        case = {"op": op, "packing": name, "bits": bits, "siting": siting, "us": med[key] * 1e3, "spread": spread[key],
                "TBps": moved[key] / (med[key] * 1e-3) / 1e12}
        if key in twin:
            t = twin[key]
            case.update({"yardstick": "/".join(str(v) for v in t), "ratio": med[key] / med[t], "byte_ratio": moved[key] / moved[t]})
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    assert all(c["us"] > 0 for c in res["cases"])


if __name__ == "__main__":
    main()
