"""The streaming session (PFNL.open_stream, include/pfnl_hip.h pfnl_stream_*) against the harness on the same box, in one job.

  python tools/stream_timing.py [--repeats 3] [--out FILE]

Sequences: 41 frames of 144x180 (a Vid4 size) and 16 frames of 270x480 (-> 1080p), the full 20-block model, synthetic weights.
  session: uint8 numpy frames pushed one at a time at batch = 1, 4, 8.  DEVICE time per SR frame = HIP events on the session's stream
           from the delivery of the first batch to the end of the sequence, over the frames of the batches launched after that point
           (window gather, pfnl_forward, quantisation and whatever the stream idles in between); WALL time per frame over the same span.
  harness: test_video_lr on the 144x180 sequence as PNGs with `part` chosen so that num_once = 1 and 4: the average the harness prints
           (HIP events per batch, gather .. D2H of the uint8 frames, first batch excluded) over num_once, `--repeats` times: the spread.
Every step is a child process under its own `timeout`; the first non-zero status ends the run."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEQS = {"144x180": (41, 144, 180), "270x480": (16, 270, 480)}


def _sequence(name):
    import numpy as np
    F, H, W = SEQS[name]
    base = np.random.default_rng(0).integers(0, 256, size=(H + 2 * F, W + 2 * F, 3), dtype=np.uint8)
    return np.stack([np.ascontiguousarray(base[i:i + H, 2 * i:2 * i + W]) for i in range(F)])


def _model(precision):
    from model.pfnl import PFNL
    from pfnl_amd import synth
    from pfnl_amd.spec import PFNLGeometry
    m = PFNL()
    m.precision = precision
    m.save_dir = os.path.join(ROOT, "no_checkpoint_here")
    m.set_weights(synth.synthetic_weights(PFNLGeometry(), seed=0))
    return m


def step_session(seq, batch, precision, repeats):
    import torch
    frames = _sequence(seq)
    F, H, W = SEQS[seq]
    m = _model(precision)
    with m.open_stream(H, W, batch) as vs:
        for rep in range(repeats + 1):                                # (the first pass warms up: allocations, first-call costs)
            n, e0, e1, t0 = 0, torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), None
            for f in list(frames) + [None]:
                got = vs.push(f) if f is not None else vs.end()
                n += len(got)
                if t0 is None and n >= min(batch, F):                 # the first batch has been delivered
                    e0.record()                                       # (behind the batch this push may have launched: it is not counted)
                    t0, n0 = time.perf_counter(), n + (vs.ready() if f is not None else 0)
            e1.record()
            e1.synchronize()
            wall = time.perf_counter() - t0
            assert n == F
            vs.reset()
            if rep and F > n0:
                print("session %s %s batch=%d: device %.3f ms / frame, wall %.3f ms / frame (%d frames)" % (
                    seq, precision, batch, e0.elapsed_time(e1) / (F - n0), 1e3 * wall / (F - n0), F - n0), flush=True)


def step_harness(seq, num_once, precision, repeats):
    import contextlib
    import io
    import re
    import tempfile
    from PIL import Image
    frames = _sequence(seq)
    F = frames.shape[0]
    part = -(-F // num_once)
    assert (F // part if F % part == 0 else F // part + 1) == num_once
    d = tempfile.mkdtemp()
    os.makedirs(os.path.join(d, "blur4"))
    for i, im in enumerate(frames):
        Image.fromarray(im).save(os.path.join(d, "blur4", "%04d.png" % i))
    m = _model(precision)
    for rep in range(repeats + 1):
        buf = io.StringIO()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(buf):
            m.test_video_lr(d, name="out", part=part)
        wall = time.perf_counter() - t0
        avg = float(re.search(r"and ([0-9.eE+-]+) s in average", buf.getvalue()).group(1))
        if rep:
            print("harness %s %s num_once=%d (part=%d): device %.3f ms / frame (per batch %.3f ms), wall of the whole call %.3f ms / frame "
                  "(PNG decode and encode included)" % (seq, precision, num_once, part, 1e3 * avg / num_once, 1e3 * avg, 1e3 * wall / F),
                  flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--step", nargs=3, default=None, metavar=("KIND", "SEQ", "N"), help="(internal) run one step in this process")
    a = ap.parse_args()
    if a.step:
        kind, seq, n = a.step
        (step_session if kind == "session" else step_harness)(seq, int(n), a.precision, a.repeats)
        return 0
    steps = [("harness", "144x180", 1), ("session", "144x180", 1), ("harness", "144x180", 4), ("session", "144x180", 4),
             ("session", "144x180", 8), ("session", "270x480", 1), ("session", "270x480", 4), ("session", "270x480", 8)]
    for kind, seq, n in steps:
        cmd = ["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--repeats", str(a.repeats), "--precision", a.precision,
               "--step", kind, seq, str(n)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith(("session", "harness"))]
        print("\n".join(lines), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        if r.returncode != 0:
            print("step %s %s %d ended with status %d: stopping\n%s" % (kind, seq, n, r.returncode, r.stderr[-2000:]), flush=True)
            return r.returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
