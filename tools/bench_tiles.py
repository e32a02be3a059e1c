"""What a tiled forward costs and saves (DESIGN.md "Tiles"; include/pfnl_hip.h TILES).  Workloads: one clip of 7x270x480 (fp32) and one of
7x540x960 (fp32 and bf16), the reference geometry (20 blocks), device tensors, HIP events, everything in one process, plain and tiled
forwards alternating over --rounds rounds after a warm-up of every shape.  Per workload and tiling (pad = 4 + 2 num_block = 44):
  total      forward(x) against forward(x, tile=...)
  nonlocal   the non-local class (nl_pack + nl_attn) of both, read through pfnl_profile_read in a pass of its own
  tiles      the tile count and the LR pixels the tiles hold over the frame's (the recomputed margin)
  kernels    pfnl_op_tile_gather and pfnl_op_tile_scatter over all tiles, in GB/s of the bytes they read and write, next to one
             device-to-device copy (torch's contiguous same-type copy_: hipMemcpyAsync) of the same bytes
  psnr       of the tiled against the whole-frame result on the synthetic clip: the price of the tile-local non-local block
usage: python tools/bench_tiles.py [--rounds 5] [--reps 3] [--sizes 270x480,540x960] [--out result.json]"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="calls inside one timed window")
    ap.add_argument("--sizes", default="270x480,540x960")
    ap.add_argument("--num-block", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from pfnl_amd import ops, synth, tiles
    from pfnl_amd.engine import PFNLEngine
    from pfnl_amd.spec import PFNLGeometry
    geom = PFNLGeometry(num_block=a.num_block)
    T, s, pad = geom.num_frames, geom.scale, 4 + 2 * geom.num_block
    eng = PFNLEngine(geom, device=0)
    eng.load_weights(synth.synthetic_weights(geom, seed=0))
    res = {"device": torch.cuda.get_device_name(0), "cus": torch.cuda.get_device_properties(0).multi_processor_count, "rounds": a.rounds,
           "reps": a.reps, "num_block": geom.num_block, "pad": pad, "cases": []}

    def timed(work):
        for f in work.values():                                                  # every shape and every launch once, twice
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
        return {k: statistics.median(v) for k, v in ms.items()}

    def nonlocal_ms(f):
        eng.profile(1)
        f()
        torch.cuda.synchronize()
        eng.profile_reset()
        for _ in range(a.reps):
            f()
        torch.cuda.synchronize()
        p = eng.profile_read()
        eng.profile(0)
        return (p["nl_pack"]["ms"] + p["nl_attn"]["ms"]) / a.reps

    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        x = torch.from_numpy(synth.uniform_clips(1, T, H, W, seed=1)).cuda()
        halves = ((H // 2 + 1) // 2 * 2 + pad + 1) // 2 * 2, ((W // 2 + 1) // 2 * 2 + pad + 1) // 2 * 2   # two tiles per axis
        tilings = [t for t in ((270, 480, pad), (136, 240, pad), halves + (pad,)) if len(tiles.axis(H, t[0], pad)) * len(tiles.axis(W, t[1], pad)) > 1]
        for precision in (("fp32",) if H * W <= 270 * 480 else ("fp32", "bf16")):
            eng.set_option("precision", precision)
            whole = eng.forward(x)
            for t in dict.fromkeys(tilings):
                th, tw, rows, cols = tiles.grid(H, W, t)
                n = len(rows) * len(cols)
                work = {"plain": lambda: eng.forward(x), "tiled": lambda: eng.forward(x, tile=t)}
                med = timed(work)
                case = {"frame": f"1x{T}x{H}x{W}", "precision": precision, "tile": list(t), "tile_shape": [th, tw], "tiles": n,
                        "pixels_over_frame": n * th * tw / (H * W), "plain_ms": med["plain"], "tiled_ms": med["tiled"],
                        "plain_nonlocal_ms": nonlocal_ms(work["plain"]), "tiled_nonlocal_ms": nonlocal_ms(work["tiled"]),
                        "psnr_tiled_vs_whole_dB": synth.psnr(eng.forward(x, tile=t).cpu().numpy(), whole.cpu().numpy())}
                if precision == "fp32":                                          # the two kernels move fp32 in both precisions: once
                    stack = ops.tile_gather(x, t)
                    y = torch.empty((n, s * th, s * tw, 3), dtype=torch.float32, device="cuda").normal_()
                    out = torch.empty_like(whole)
                    g_bytes, s_bytes = 2 * 4 * stack.numel(), 2 * 4 * out.numel()
                    g_src, s_src = (torch.empty(b // 2, dtype=torch.uint8, device="cuda") for b in (g_bytes, s_bytes))
                    g_dst, s_dst = torch.empty_like(g_src), torch.empty_like(s_src)
                    k = timed({"gather": lambda: ops.tile_gather(x, t, out=stack), "gather_copy": lambda: g_dst.copy_(g_src),
                               "scatter": lambda: ops.tile_scatter(y, out, t, s), "scatter_copy": lambda: s_dst.copy_(s_src)})
                    case.update({"gather_ms": k["gather"], "scatter_ms": k["scatter"],
                                 "gather_GBps": g_bytes / (k["gather"] * 1e-3) / 1e9, "gather_copy_GBps": g_bytes / (k["gather_copy"] * 1e-3) / 1e9,
                                 "scatter_GBps": s_bytes / (k["scatter"] * 1e-3) / 1e9, "scatter_copy_GBps": s_bytes / (k["scatter_copy"] * 1e-3) / 1e9})
                    del stack, y, out, g_src, s_src, g_dst, s_dst
                res["cases"].append(case)
                print(json.dumps(case), flush=True)
        eng.set_option("precision", "fp32")
    eng.sync()
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    eng.close()
    assert all(np.isfinite(c["tiled_ms"]) for c in res["cases"])


if __name__ == "__main__":
    main()
