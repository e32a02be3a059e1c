"""The cold start of tests/test_gpu_threads.py part E, as a program of its own: `python threads_cold.py SHAPES.json OUT.npz`.

Every other thread test runs after a serial pass has set every kernel attribute, filled every lazy per-device cache (common.h
device_cu_count, the launchers' attr_dev tables) and uploaded c_blur - the races the launchers' comments speak of ("a racing first call
repeats the same upload") happen on FIRST use only.  Here the first library calls of a fresh process are four threads at once: each
creates its own engine, loads its weights and runs one forward (small, chain, bf16), the fourth runs blur_decimate and bicubic.  One round,
no warm-up.  The results and the stamps go to OUT.npz; the parent compares them bit for bit with its own serial results.

The parent imports this module for the workers' inputs, so that both sides build them by the same lines."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import history as Hy  # noqa: E402
import threads as Th  # noqa: E402

NB = 2                                            # PF blocks, as tests/test_gpu_history.py
FAMILIES = ("small", "chain", "bf16")
HR_SHAPE, LR_SHAPE, SCALE = (2, 45, 70, 3), (2, 16, 24, 3), 4
CHILD_TIMEOUT_S = 120.0                           # run_together's limit inside the child: engine creation, weights and one forward each


def family_target(family: str) -> Hy.Target:
    return next(t for t in Hy.family_targets() if t.family == family)


def clip(t: Hy.Target, shape) -> np.ndarray:
    """tests/test_gpu_history.py _case's clip of the target: the parent judges its serial result against the oracle result cached there."""
    from pfnl_amd import synth
    B, H, W = shape
    return synth.uniform_clips(B, t.T, H, W, seed=11 + B)


def weights(t: Hy.Target):
    from pfnl_amd import synth
    from pfnl_amd.spec import PFNLGeometry
    return synth.synthetic_weights(PFNLGeometry(num_frames=t.T, num_block=NB), seed=0)


def op_inputs():
    rng = np.random.default_rng(45)
    return rng.random(HR_SHAPE, dtype=np.float32), rng.random(LR_SHAPE, dtype=np.float32)


def forward_worker(t: Hy.Target, x_dev, stream):
    """A worker whose call creates the engine, loads the weights, sets the target's options on top of the library's defaults and runs one
    device-pointer forward on `stream`."""
    import torch
    from pfnl_amd.engine import PFNLEngine
    from pfnl_amd.spec import PFNLGeometry

    def work(r):
        eng = PFNLEngine(PFNLGeometry(num_frames=t.T, num_block=NB), device=0)
        eng.load_weights(weights(t))
        for k, v in t.options:
            eng.set_option(k, v)
        with torch.cuda.stream(stream):
            y = eng.forward(x_dev)
            stream.synchronize()
            eng.sync()
            out = y.cpu().numpy()
        structure = eng.plan(*x_dev.shape[:1], *x_dev.shape[2:4])["structure"]
        eng.close()
        return out, structure
    return work


def ops_worker(hr_dev, lr_dev, stream):
    import torch
    from pfnl_amd import ops

    def work(r):
        with torch.cuda.stream(stream):
            a = ops.blur_decimate(hr_dev, SCALE)
            b = ops.bicubic(lr_dev, SCALE)
            stream.synchronize()
            return a.cpu().numpy(), b.cpu().numpy()
    return work


def main(shapes_path: str, out_path: str) -> int:
    import torch
    with open(shapes_path) as f:
        shapes = {k: tuple(v) for k, v in json.load(f).items()}                   # family -> (B, H, W); a family out of reach is absent
    from pfnl_amd import _capi
    torch.cuda.init()
    _capi.load_library()                                                        # loaded and typed, but no call into it before the threads
    workers = {}
    for fam in FAMILIES:
        if fam in shapes:
            t = family_target(fam)
            workers[fam] = forward_worker(t, torch.from_numpy(clip(t, shapes[fam])).cuda(), torch.cuda.Stream())
    hr, lr = op_inputs()
    workers["ops"] = ops_worker(torch.from_numpy(hr).cuda(), torch.from_numpy(lr).cuda(), torch.cuda.Stream())
    torch.cuda.synchronize()
    run = Th.run_together(workers, rounds=1, timeout_s=CHILD_TIMEOUT_S)
    out = {}
    for name in run.names:
        out["stamps_" + name] = np.array(run.stamps[name][0], np.float64)
    for fam in FAMILIES:
        if fam in shapes:
            out["y_" + fam], structure = run.results[fam][0]
            out["structure_" + fam] = np.array(structure)
    out["blur"], out["bicubic"] = run.results["ops"][0]
    np.savez(out_path, **out)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
