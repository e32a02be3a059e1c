"""Film material for the inverse-telecine tests (pfnl_amd/telecine.py), shared by tests/test_telecine_host.py and tests/test_gpu_telecine.py.

``film(n, H, W, maxv, seed)``: n RGB film frames [H, W, 3] of pfnl_amd/synth.py content - the HR frame of ``moving_field_clips``, one independent
band-limited field per film frame, so every frame differs from its predecessor everywhere -, at 30 % contrast around mid-grey: smooth enough
that no sample of a true frame is combed at the default threshold (its curvature over two rows stays below it), different enough that a
weave of two film frames is combed in a large part of its samples.  The host test asserts both before the GPU tests rely on them.

``video(n, H, W, maxv, seed)``: n woven frames whose two fields come from two different instants - what a video insert is.

``candidates(h, W, maxv, seed)``: (A, Xc, Xp) for the op tests - Xc anywhere, Xp within a few thresholds of A's rows, a quarter of its
samples exactly T, T + 1 or 4 T + 1 from them, so products land on both sides of T^2 and on it; at 10 bits some samples lie above 1023."""
import numpy as np

from pfnl_amd import synth

SHAPES = ((8, 12), (16, 20))                                            # the sessions' H x W
N_FILM, N_PUSHED = 8, 10


def _dtype(maxv):
    return np.uint8 if maxv == 255 else np.uint16


def film(n=N_FILM, H=8, W=12, maxv=255, seed=7):
    _, gt = synth.moving_field_clips(n, 1, H // 4, W // 4, seed=seed)
    return [np.round((0.35 + 0.3 * gt[b]) * maxv).astype(_dtype(maxv)) for b in range(n)]


def video(n, H, W, maxv=255, seed=23):
    instants = film(2 * n, H, W, maxv, seed)
    out = []
    for i in range(n):
        f = instants[2 * i].copy()
        f[1::2] = instants[2 * i + 1][1::2]
        out.append(f)
    return out


def candidates(h, W, maxv=255, seed=0, threshold=10):
    rng = np.random.default_rng(seed + 1000 * h + W)
    T = threshold * (1 if maxv == 255 else 4)
    A = rng.integers(0, maxv + 1, (h, W, 3))
    Xc = rng.integers(0, maxv + 1, (h, W, 3))
    step = rng.choice(np.array([-4 * T - 1, -T - 1, -T, T, T + 1, 4 * T + 1]), (h, W, 3))
    Xp = np.clip(A + np.where(rng.random((h, W, 3)) < 0.25, step, rng.integers(-3 * T, 3 * T + 1, (h, W, 3))), 0, maxv)
    if maxv == 1023:
        hot = rng.random((h, W, 3)) < 0.05
        A = np.where(hot, rng.choice(np.array([1024, 2000, 32768, 65535]), (h, W, 3)), A)
        Xc = np.where(np.roll(hot, 1, axis=1), 65535, Xc)
    return tuple(v.astype(_dtype(maxv)) for v in (A, Xc, Xp))
