"""What the content box costs next to a copy of its bytes and next to the scene sum (include/pfnl_hip.h BARS;
pfnl_amd/csrc/bars.hip), and what a crop ahead of the network saves.
Workloads, one 1080 x 1920 frame at both depths: pfnl_op_content_box_* (reads the frame once) on a letterboxed frame (2.39:1 inside 16:9,
black bars: most column adds of the bars' strips are skipped) and on a frame that is picture everywhere; pfnl_op_scene_sad_* on two frames
(reads two); and IN THE SAME RUN the yardstick, a device-to-device copy of one frame's bytes (reads one, writes one).  Both hooks allocate
their scratch words, clear them and synchronise the stream in every call, so a call is more than its kernel: the table gives the call, and
the kernels' own times come from a trace of this same script (rocprofv3 --kernel-trace --stats -- python tools/bench_bars.py --reps 50
--no-session).  Device tensors, HIP events, everything in one process, the cases alternating over --rounds rounds after a warm-up of every
case.  Per case: the median microseconds of one call, its spread over the rounds (max - min) / median, and the ratio of its median to the
copy's.
Then the crop: ``upscale`` on an in-memory Y4M stream of --frames 480 x 720 frames with 2.39:1 bars (90 rows above and below 300 of
picture), with and without ``--crop auto``, alternating, wall-clock frames per second as ``upscale`` reports them.
usage: python tools/bench_bars.py [--rounds 7] [--reps 200] [--frames 24] [--no-session] [--out result.json]"""
import argparse
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 1080, 1920


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200, help="calls inside one timed window")
    ap.add_argument("--frames", type=int, default=24, help="frames of the upscale stream")
    ap.add_argument("--no-session", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import ctypes as C

    import numpy as np
    import torch
    from pfnl_amd import _capi, bars, ops, synth, y4m, yuv
    from pfnl_amd import upscale as up
    from pfnl_amd.engine import PFNLEngine
    from pfnl_amd.spec import PFNLGeometry
    lib, keep = _capi.load_library(), []
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "size": f"{H}x{W}", "cases": []}
    g = torch.Generator(device="cuda").manual_seed(1)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    work, twin = {}, {}
    top = (H - int(round(W / 2.39))) // 2 // 2 * 2                               # 138 rows of bar above and below
    for bits in (8, 10):
        raw = torch.randint(1 << (bits - 1), 1 << bits, (2, H, W, 3), dtype=torch.int16, device="cuda", generator=g)
        dark = raw.clone()                                                       # (torch fills and copies int16, not uint16)
        dark[:, :top] = 0
        dark[:, H - top:] = 0
        full, boxed = (raw.to(torch.uint8), dark.to(torch.uint8)) if bits == 8 else (raw.view(torch.uint16), dark.view(torch.uint16))
        for name, frames, want in (("letterbox", boxed, (top, 0, H - 2 * top, W)), ("full", full, (0, 0, H, W))):   # the hook against the rule, once
            box, rows, cols = ops.content_box(frames[0], 8, sums=True)
            host = frames[0].cpu().numpy() if bits == 8 else frames[0].view(torch.int16).cpu().numpy().view(np.uint16)
            r, c = bars.line_sums(host, bits)
            assert tuple(box.cpu().tolist()[0]) == want == bars.box(r, c, H, W, 8)
            assert np.array_equal(rows.view(torch.int32).cpu().numpy()[0], r) and np.array_equal(cols.view(torch.int32).cpu().numpy()[0], c)
        out_box, out_sad = torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
        src = full[0].reshape(-1).view(torch.uint8)
        dst = torch.empty_like(src)
        keep.append((full, boxed, out_box, out_sad, dst))
        cb = lib.pfnl_op_content_box_u8 if bits == 8 else lib.pfnl_op_content_box_u10
        sad = lib.pfnl_op_scene_sad_u8 if bits == 8 else lib.pfnl_op_scene_sad_u10
        copy = ("copy", bits)
        work[copy] = lambda src=src, dst=dst: dst.copy_(src)
        for name, frames in (("content_box letterbox", boxed), ("content_box full", full)):
            args = (C.c_void_p(frames[0].data_ptr()), 1, H, W, 8, C.c_void_p(out_box.data_ptr()), None, None, st)
            work[(name, bits)], twin[(name, bits)] = (lambda hook=cb, args=args: hook(*args)), copy
        args = (C.c_void_p(full[0].data_ptr()), C.c_void_p(full[1].data_ptr()), H, W, C.c_void_p(out_sad.data_ptr()), st)
        work[("scene_sad", bits)], twin[("scene_sad", bits)] = (lambda hook=sad, args=args: hook(*args)), copy

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
    for key in work:
        name, bits = key
        case = {"call": name, "bits": bits, "us": med[key] * 1e3, "spread": (max(ms[key]) - min(ms[key])) / med[key],
                "MB_per_frame": H * W * 3 * (1 if bits == 8 else 2) / 1e6}
        if key in twin:
            case["ratio_to_copy"] = med[key] / med[twin[key]]
            case["ratio_to_scene_sad"] = med[key] / med[("scene_sad", bits)]
        res["cases"].append(case)
        print(json.dumps(case), flush=True)

    if not a.no_session:                                                         # the crop: 2.39:1 bars inside 480 x 720
        sh, sw, bar = 480, 720, 90
        _, gt = synth.moving_field_clips(a.frames, 1, (sh - 2 * bar) // 4, sw // 4, seed=7)
        head = y4m.Y4MHeader(width=sw, height=sh, rate="24000:1001", interlace="p", siting="left")
        data = io.BytesIO()
        wr = y4m.Y4MWriter(data, head)
        for b in range(a.frames):
            rgb = np.zeros((sh, sw, 3), np.uint8)
            rgb[bar:sh - bar] = np.round((0.35 + 0.3 * gt[b]) * 255).astype(np.uint8)
            wr.write_frame(yuv.from_rgb(rgb, "i420", "bt601", False, "left"))
        geom = PFNLGeometry()
        eng = PFNLEngine(geom, device=0)
        eng.load_weights(synth.synthetic_weights(geom, seed=0))
        secs = {"whole": [], "crop auto": []}
        for r in range(a.rounds // 2 + 2):                                       # (the first round warms both up)
            for name, kw in (("whole", {}), ("crop auto", {"crop": "auto", "crop_probe": 12})):
                out, err = io.BytesIO(), io.StringIO()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                n = up.upscale(y4m.Y4MReader(io.BytesIO(data.getvalue())), y4m.Y4MWriter(out), eng.open_stream, log=err, batch=2, scale=geom.scale, **kw)
                torch.cuda.synchronize()
                assert n == a.frames and (name == "whole" or err.getvalue().startswith(f"crop {bar},0,{sh - 2 * bar},{sw} (from 12 frames)"))
                if r:
                    secs[name].append(time.perf_counter() - t0)
        eng.close()
        t = {k: statistics.median(v) for k, v in secs.items()}
        res["upscale"] = {"size": f"{sh}x{sw}", "picture": f"{sh - 2 * bar}x{sw}", "frames": a.frames, "runs": len(secs["whole"]),
                          "fps_whole": a.frames / t["whole"], "fps_crop_auto": a.frames / t["crop auto"], "speedup": t["whole"] / t["crop auto"],
                          "rows_kept": (sh - 2 * bar) / sh}
        print(json.dumps(res["upscale"]), flush=True)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    assert all(c["us"] > 0 for c in res["cases"])


if __name__ == "__main__":
    main()
