"""What the self-ensemble costs (DESIGN.md "Self-ensemble"; include/pfnl_hip.h SELF-ENSEMBLE).  Workload: BASELINE.json configs[1]'s
batch, 4 clips of 7x128x128, the reference geometry (20 blocks), device tensors, HIP events, everything in one process, the four
measurements alternating over --rounds rounds after a warm-up of every shape:
  ensemble   forward(x, ensemble=8)
  forwards   the yardstick: 8 plain forwards of that batch, 4 on x and 4 on the pre-transposed input
  kernels    the two new kernels alone: members 1 .. 7 of pfnl_op_dihedral on the input tensor and of pfnl_op_dihedral_accum on the
             output tensor
  copy       one device-to-device hipMemcpyAsync (torch's contiguous same-type copy_) that moves the bytes those 14 launches move:
             7 x (read + write the input tensor) + 7 x (read the member's output, read and write the sum); a copy of N bytes moves 2 N
  copy14     those bytes as 14 copies, one per launch of `kernels`: what the launch count alone costs
  mirrors6 / transposes8   `kernels` split by path: members 1 .. 3 (whole pixels in 16-byte words) and 4 .. 7 (through the LDS tile)
usage: python tools/bench_ensemble.py [--rounds 7] [--reps 5] [--out result.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5, help="calls inside one timed window")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from pfnl_amd import ops, synth
    from pfnl_amd.engine import PFNLEngine
    from pfnl_amd.spec import PFNLGeometry
    geom = PFNLGeometry()
    B, T, H, W, s = 4, geom.num_frames, 128, 128, geom.scale
    eng = PFNLEngine(geom, device=0)
    eng.load_weights(synth.synthetic_weights(geom, seed=0))
    x = torch.from_numpy(synth.uniform_clips(B, T, H, W, seed=1)).cuda()
    xt = ops.dihedral(x, 4)                                                      # the pre-transposed input of the yardstick
    y = eng.forward(x)
    acc = torch.zeros_like(y)
    n_in, n_out = x.numel(), y.numel()
    moved = 4 * (7 * 2 * n_in + 7 * 3 * n_out)                                   # bytes the 14 launches read and write
    src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)

    def ensemble8():
        eng.forward(x, ensemble=8)

    def forwards8():
        for _ in range(4):
            eng.forward(x)
            eng.forward(xt)

    def kernels14():
        for k in range(1, 8):
            ops.dihedral(x, k, out=xt if k & 4 else x2)
        for k in range(1, 8):
            ops.dihedral_accum(acc, yt if k & 4 else y, k, 0.125 if k == 7 else 1.0)

    def copy():
        dst.copy_(src)

    def copy14():                                                                # the same bytes as 14 copies, one per launch
        for _ in range(7):
            dst[:4 * n_in].copy_(src[:4 * n_in])
        for _ in range(7):
            dst[:6 * n_out].copy_(src[:6 * n_out])

    def mirrors6():                                                              # members 1 .. 3 of both kernels
        for k in range(1, 4):
            ops.dihedral(x, k, out=x2)
            ops.dihedral_accum(acc, y, k, 1.0)

    def transposes8():                                                           # members 4 .. 7 of both kernels
        for k in range(4, 8):
            ops.dihedral(x, k, out=xt)
            ops.dihedral_accum(acc, yt, k, 1.0)

    x2 = torch.empty_like(x)
    yt = ops.dihedral(y, 4)
    work = {"ensemble": ensemble8, "forwards": forwards8, "kernels": kernels14, "copy": copy, "copy14": copy14, "mirrors6": mirrors6,
            "transposes8": transposes8}
    for f in work.values():                                                      # every shape and every launch once, twice
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
    eng.sync()
    res = {"workload": f"{B}x{T}x{H}x{W}, num_block={geom.num_block}, fp32", "device": torch.cuda.get_device_name(0),
           "cus": torch.cuda.get_device_properties(0).multi_processor_count, "rounds": a.rounds, "reps": a.reps, "bytes_moved": moved}
    for name, v in ms.items():
        res[name + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        print("%-9s median %.3f ms (min %.3f, max %.3f)" % (name, res[name + "_ms"]["median"], min(v), max(v)), flush=True)
    med = {k: res[k + "_ms"]["median"] for k in work}
    res["ensemble_minus_forwards_ms"] = med["ensemble"] - med["forwards"]
    res["kernels_over_copy"] = med["kernels"] / med["copy"]
    res["copy_GBps_of_bytes_moved"] = moved / (med["copy"] * 1e-3) / 1e9
    res["kernels_GBps_of_bytes_moved"] = moved / (med["kernels"] * 1e-3) / 1e9
    res["hr_frames_per_s_ensemble8"] = B / (med["ensemble"] * 1e-3)
    res["kernels_over_copy14"] = med["kernels"] / med["copy14"]
    res["mirrors_GBps_of_bytes_moved"] = moved * 3 / 7 / (med["mirrors6"] * 1e-3) / 1e9
    res["transposes_GBps_of_bytes_moved"] = moved * 4 / 7 / (med["transposes8"] * 1e-3) / 1e9
    print("kernels / copy14 %.2f; mirrors %.0f GB/s, transposes %.0f GB/s of the bytes they move" % (
        res["kernels_over_copy14"], res["mirrors_GBps_of_bytes_moved"], res["transposes_GBps_of_bytes_moved"]), flush=True)
    print("ensemble - forwards %.3f ms; kernels / copy %.2f; %.0f GB/s (copy) vs %.0f GB/s (kernels) of %d bytes moved" % (
        res["ensemble_minus_forwards_ms"], res["kernels_over_copy"], res["copy_GBps_of_bytes_moved"], res["kernels_GBps_of_bytes_moved"], moved), flush=True)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    eng.close()
    assert np.isfinite(list(med.values())).all()


if __name__ == "__main__":
    main()
