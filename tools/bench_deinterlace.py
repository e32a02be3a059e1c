"""What the deinterlacer costs next to a copy of its bytes (include/pfnl_hip.h INTERLACED; pfnl_amd/csrc/deinterlace.hip).
Workloads: the one-frame launch (five fields in, one progressive frame out: 2.5 frames read, 1 written) and the two-frame launch of a
field-rate push (six fields in, two frames out: each launch's blocks read their own five, 5 frames read in all, 2 written) at 480 x 720,
576 x 720 and 1080 x 1920, at both depths, and IN THE SAME RUN the yardstick of each: a device-to-device copy of the bytes the kernel
reads and writes, half of them each way.  Device tensors, HIP events, everything in one process, the cases alternating over --rounds
rounds after a warm-up of every case; the hooks are called with arguments made once (ops.py's checks cost more host time per call than
a small frame takes).  Per case: the median microseconds of one call, its spread over the rounds (max - min) / median,
the TB/s of the bytes it reads and writes, and the ratio of its median to the copy's.
usage: python tools/bench_deinterlace.py [--rounds 7] [--reps 300] [--out result.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = ((480, 720), (576, 720), (1080, 1920))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=300, help="calls inside one timed window")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import ctypes as C
    from pfnl_amd import _capi, ops
    lib, keep = _capi.load_library(), []
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "cases": []}
    g = torch.Generator(device="cuda").manual_seed(1)
    work, moved, twin = {}, {}, {}
    for H, W in SIZES:
        for bits in (8, 10):
            sz = 1 if bits == 8 else 2
            raw = torch.randint(0, 1 << bits, (6, H // 2, W, 3), dtype=torch.int16, device="cuda", generator=g)
            fields = list(raw.to(torch.uint8) if bits == 8 else raw.view(torch.uint16))
            frame = H * W * 3 * sz
            one = torch.empty((H, W, 3), dtype=fields[0].dtype, device="cuda")
            two = torch.empty((2, H, W, 3), dtype=fields[0].dtype, device="cuda")
            assert torch.equal(ops.deinterlace_pair(fields, 0)[0], (ops.deinterlace if bits == 8 else ops.deinterlace_u10)(*fields[:5], 0))
            # the hooks themselves, their arguments made once: ops.py's checks cost more host time per call than the small frames take
            hook1, hook2 = (lib.pfnl_op_deinterlace_u8, lib.pfnl_op_deinterlace_pair_u8) if bits == 8 else \
                (lib.pfnl_op_deinterlace_u10, lib.pfnl_op_deinterlace_pair_u10)
            ptr = [C.c_void_p(f.data_ptr()) for f in fields]
            six, st = (C.c_void_p * 6)(*ptr), C.c_void_p(torch.cuda.current_stream().cuda_stream)
            keep.append((fields, one, two, six))
            a1 = (*ptr[:5], H, W, 0, C.c_void_p(one.data_ptr()), st)
            a2 = (six, H, W, 0, C.c_void_p(two.data_ptr()), st)
            for launch, f, nbytes in (("one", lambda hook=hook1, args=a1: hook(*args), 7 * frame // 2),
                                      ("two", lambda hook=hook2, args=a2: hook(*args), 7 * frame)):
                key = (launch, H, W, bits)
                work[key], moved[key], twin[key] = f, nbytes, ("copy-" + launch, H, W, bits)
                src, dst = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda"), torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
                work[twin[key]], moved[twin[key]] = (lambda src=src, dst=dst: dst.copy_(src)), 2 * (nbytes // 2)

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
        launch, H, W, bits = key
        case = {"launch": launch, "size": f"{H}x{W}", "bits": bits, "us": med[key] * 1e3, "spread": spread[key], "MB": moved[key] / 1e6,
                "TBps": moved[key] / (med[key] * 1e-3) / 1e12}
        if key in twin:
            case["ratio"] = med[key] / med[twin[key]]
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
