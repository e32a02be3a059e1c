"""What scenes cost the streaming session (pfnl_stream_scenes), on one box, in one process.

  python tools/scene_timing.py [--repeats 3]            wall time per delivered frame, 64 frames of 144x180 at batch 4, the 20-block
                                                        model: scene_cut off and at threshold 10, alternating, `--repeats` times each
  python tools/scene_timing.py --kernels                pushes 16 frames each of 144x180 and 270x480 through a one-block session with the
                                                        detector on and prints nothing: for `rocprofv3 --kernel-trace --stats -- python ...`
                                                        (stream_scene_sad_kernel against stream_gather_u8_scenes_kernel, per frame size)"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _sequence(F, H, W):
    """a one-pixel-per-frame pan over an image of random 16x16 blocks, and another image (a cut) every 16 frames"""
    import numpy as np
    rng = np.random.default_rng(0)
    out = []
    for f in range(F):
        if f % 16 == 0:
            blocks = rng.integers(0, 256, size=(H // 16 + 1, W // 16 + 2, 3), dtype=np.uint8)
            base = np.kron(blocks, np.ones((16, 16, 1), np.uint8))
        out.append(np.ascontiguousarray(base[:H, f % 16:f % 16 + W]))
    return np.stack(out)


def _engine(num_block):
    from pfnl_amd import synth
    from pfnl_amd.engine import PFNLEngine
    from pfnl_amd.spec import PFNLGeometry
    geom = PFNLGeometry(num_block=num_block)
    eng = PFNLEngine(geom, device=0)
    eng.load_weights(synth.synthetic_weights(geom, seed=0))
    return eng


def run_session(eng, frames, batch, scene_cut):
    """(seconds per delivered frame from the first delivery to the last, cuts)"""
    F, H, W = frames.shape[:3]
    with eng.open_stream(H, W, batch, scene_cut=scene_cut) as vs:
        n, t0, n0 = 0, None, 0
        for f in list(frames) + [None]:
            n += len(vs.push(f) if f is not None else vs.end())
            if t0 is None and n:
                t0, n0 = time.perf_counter(), n
        wall = time.perf_counter() - t0
        assert n == F
        return wall / (F - n0), list(vs.cuts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    if a.kernels:
        eng = _engine(1)
        for H, W in ((144, 180), (270, 480)):
            run_session(eng, _sequence(16, H, W), 4, 10.0)
        eng.close()
        return 0
    eng = _engine(20)
    frames = _sequence(64, 144, 180)
    run_session(eng, frames, 4, None)                                 # warm-up: allocations, first-call costs
    run_session(eng, frames, 4, 10.0)
    for rep in range(a.repeats):
        for cut in (None, 10.0):
            per, cuts = run_session(eng, frames, 4, cut)
            print("session 144x180 batch=4 scene_cut=%s rep %d: wall %.3f ms / frame, cuts %s" % (cut, rep, 1e3 * per, cuts), flush=True)
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
