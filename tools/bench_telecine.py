"""What inverse telecine costs next to a copy of its bytes and next to the deinterlacer (include/pfnl_hip.h TELECINE;
pfnl_amd/csrc/telecine.hip).  Workloads, at 1080 x 1920 and both depths: the two launches a session issues per matched frame
(pfnl_op_telecine_frame_* with post = 0, so that no frame is flagged and the weave always reads and writes - asserted on the decision the
timed calls leave: the match reads A, Xc, Xp - 1.5 frames -, the weave reads A and the chosen partner and writes the frame - 1 frame
each way: 2.5 frames read, 1 written); the match alone on a flagged frame (post = 1 on these random fields: the weave launch finds
nothing to do), which is what the match and an empty launch cost; the device-to-device copy of one frame that mode "decimate" adds per
delivered frame; pfnl_op_deinterlace_* on the same fields (2.5 frames read, 1 written); and IN THE SAME RUN the
yardstick: a device-to-device copy of as many bytes, half of them each way.  Device tensors, HIP events, everything in one process, the
cases alternating over --rounds rounds after a warm-up of every case; the hooks are called with arguments made once.  Per case: the median
microseconds of one call, its spread over the rounds (max - min) / median, the TB/s of the bytes it reads and writes, and the ratio of its
median to the copy's.
Then a session both ways: 10 pushed frames of 3:2 material at --session-size through a "decimate" session (8 forwards) and through an
interlaced="frame" session (10 forwards), wall-clock from the first push to the last pop, the median of --rounds runs each.
usage: python tools/bench_telecine.py [--rounds 7] [--reps 300] [--session-size 128x192] [--out result.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 1080, 1920


def _session_seconds(eng, pushed, size, rounds, **kw):
    import torch
    secs, frames = [], 0
    with eng.open_stream(size[0], size[1], 2, **kw) as vs:
        for r in range(rounds + 1):                                               # (the first run warms up)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            frames = 0
            for f in pushed:
                frames += len(vs.push(f))
            frames += len(vs.end())
            torch.cuda.synchronize()
            if r:
                secs.append(time.perf_counter() - t0)
            vs.reset()
    return statistics.median(secs), frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=300, help="calls inside one timed window")
    ap.add_argument("--session-size", default="128x192")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import ctypes as C

    import numpy as np
    import torch
    from pfnl_amd import _capi, ops, synth, telecine
    from pfnl_amd.engine import PFNLEngine
    from pfnl_amd.spec import PFNLGeometry
    lib, keep = _capi.load_library(), []
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "reps": a.reps, "size": f"{H}x{W}", "cases": []}
    g = torch.Generator(device="cuda").manual_seed(1)
    work, moved, twin, decisions = {}, {}, {}, {}
    for bits in (8, 10):
        sz = 1 if bits == 8 else 2
        raw = torch.randint(0, 1 << bits, (5, H // 2, W, 3), dtype=torch.int16, device="cuda", generator=g)
        fields = list(raw.to(torch.uint8) if bits == 8 else raw.view(torch.uint16))
        frame = H * W * 3 * sz
        out = torch.empty((H, W, 3), dtype=fields[0].dtype, device="cuda")
        words = torch.zeros(6, dtype=torch.int64, device="cuda")
        got, d = ops.telecine_frame(fields[2], fields[3], fields[1], 0)           # (the hook against the rule on these fields, once)
        host = [f.cpu().numpy() if bits == 8 else f.view(torch.int16).cpu().numpy().view(np.uint16) for f in fields]
        which, cc, cp = telecine.match(host[2], host[3], host[1], 0, 10, (1 << bits) - 1)
        assert (d["count_c"], d["count_p"], d["match"]) == (cc, cp, int(which == "p"))
        ptr = [C.c_void_p(f.data_ptr()) for f in fields]
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        keep.append((fields, out, words))
        tc = lib.pfnl_op_telecine_frame_u8 if bits == 8 else lib.pfnl_op_telecine_frame_u10
        di = lib.pfnl_op_deinterlace_u8 if bits == 8 else lib.pfnl_op_deinterlace_u10
        no_post, post = _capi.pfnl_telecine_params(10, 0, -1), _capi.pfnl_telecine_params(10, 1, -1)
        words_post = torch.zeros(6, dtype=torch.int64, device="cuda")
        keep.append((no_post, post, words_post))
        a_tc = (ptr[2], ptr[3], ptr[1], H // 2, W, 0, C.byref(no_post), C.c_void_p(out.data_ptr()), C.c_void_p(words.data_ptr()), st)
        a_fl = (ptr[2], ptr[3], ptr[1], H // 2, W, 0, C.byref(post), C.c_void_p(out.data_ptr()), C.c_void_p(words_post.data_ptr()), st)
        decisions[bits] = (words, words_post)
        a_di = (*ptr, H, W, 0, C.c_void_p(out.data_ptr()), st)
        assert tc(*a_tc) == 0 and di(*a_di) == 0, lib.pfnl_last_error()
        nbytes = 7 * frame // 2
        src, dst = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda"), torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
        copy = ("copy", bits)
        work[copy], moved[copy] = (lambda src=src, dst=dst: dst.copy_(src)), 2 * (nbytes // 2)
        for name, f in (("match+weave", lambda hook=tc, args=a_tc: hook(*args)), ("deinterlace", lambda hook=di, args=a_di: hook(*args))):
            work[(name, bits)], moved[(name, bits)], twin[(name, bits)] = f, nbytes, copy
        work[("match, flagged", bits)], moved[("match, flagged", bits)] = (lambda hook=tc, args=a_fl: hook(*args)), 3 * frame // 2
        one, ring = torch.empty(frame, dtype=torch.uint8, device="cuda"), torch.empty(frame, dtype=torch.uint8, device="cuda")
        work[("ring copy", bits)], moved[("ring copy", bits)] = (lambda src=one, dst=ring: dst.copy_(src)), 2 * frame

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
    for bits, (words, words_post) in decisions.items():                          # what the timed calls decided: the weave ran, or did not
        d, f = [int(v) for v in words.cpu()], [int(v) for v in words_post.cpu()]
        assert d[3] == 0 and f[3] == 1 and d[:3] == f[:3] and d[4:] == f[4:] == [0, 0], (bits, d, f)
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: (max(v) - min(v)) / med[k] for k, v in ms.items()}
    for key in work:
        name, bits = key
        case = {"launch": name, "bits": bits, "us": med[key] * 1e3, "spread": spread[key], "MB": moved[key] / 1e6,
                "TBps": moved[key] / (med[key] * 1e-3) / 1e12}
        if key in twin:
            case["ratio_to_copy"] = med[key] / med[twin[key]]
            if name == "match+weave":
                case["ratio_to_deinterlace"] = med[key] / med[("deinterlace", bits)]
        res["cases"].append(case)
        print(json.dumps(case), flush=True)

    # a session of 10 pushed frames both ways
    size = tuple(int(v) for v in a.session_size.lower().split("x"))
    geom = PFNLGeometry()
    eng = PFNLEngine(geom, device=0)
    eng.load_weights(synth.synthetic_weights(geom, seed=0))
    _, gt = synth.moving_field_clips(8, 1, size[0] // 4, size[1] // 4, seed=7)
    film = [np.round((0.35 + 0.3 * gt[b]) * 255).astype(np.uint8) for b in range(8)]
    pushed = [torch.from_numpy(f).cuda() for f in telecine.pulldown(film, 0, "tff")]
    t_tc, n_tc = _session_seconds(eng, pushed, size, a.rounds, telecine="decimate")
    t_di, n_di = _session_seconds(eng, pushed, size, a.rounds, interlaced="frame")
    eng.close()
    res["session"] = {"size": a.session_size, "pushed": len(pushed), "decimate": {"frames": n_tc, "ms": t_tc * 1e3},
                      "deinterlace_frame": {"frames": n_di, "ms": t_di * 1e3}, "ratio": t_tc / t_di}
    print(json.dumps(res["session"]), flush=True)
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    assert all(c["us"] > 0 for c in res["cases"]) and (n_tc, n_di) == (8, 10)


if __name__ == "__main__":
    main()
