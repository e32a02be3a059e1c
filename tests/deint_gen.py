"""Woven test sequences for the deinterlacer (pfnl_amd/deinterlace.py), shared by tests/test_deinterlace_host.py and
tests/test_gpu_deinterlace.py: content that reaches every case of the rule at the small shapes the tests use.

``woven_rgb(n, H, W, maxv, seed)``: n RGB frames [H, W, 3] (uint8 for maxv 255, uint16 for 1023) -
  * a random base scrolled one row per frame, plus noise of +-3: the picture moves, the cubic and the clamp both decide;
  * frame 2 repeats frame 1: nothing moves there, diff reaches 0 and the made row is the weave;
  * the last frame is blocks of 0 / MAX whose field rows read MAX 0 0 MAX in one column block and 0 MAX MAX 0 in the next: the cubic's
    numerator falls below 0 and rises above 16 MAX.
``branch_counts`` sums deinterlace.branches over every field of the sequence; SEED is one for which every count is above 0 at 8 x 6 and
12 x 22 at both depths (asserted by the host test)."""
import numpy as np

from pfnl_amd import deinterlace

SEED = 1
SHAPES = ((8, 6), (12, 22))


def woven_rgb(n, H, W, maxv=255, seed=SEED):
    rng = np.random.default_rng(seed)
    dtype = np.uint8 if maxv == 255 else np.uint16
    base = rng.integers(0, maxv + 1, (H + n, W, 3)).astype(np.int32)
    frames = []
    for i in range(n):
        noise = rng.integers(-3, 4, (H, W, 3))
        frames.append(np.clip(base[i:i + H] + noise, 0, maxv).astype(dtype))
    if n > 2:
        frames[2] = frames[1].copy()
    if n > 1:
        y, x = np.arange(H)[:, None] // 2, np.arange(W)[None, :] // 2
        on = np.isin((y + 2 * (x % 2)) % 4, (0, 3))
        frames[-1] = np.repeat((on * maxv).astype(dtype)[:, :, None], 3, axis=2)
    return frames


def branch_counts(frames, field_order="tff", maxv=255):
    seq = deinterlace.sequence_fields(frames, field_order)
    total = dict.fromkeys(deinterlace.BRANCHES, 0)
    for k in range(len(seq)):
        a, b, c, d = deinterlace.neighbours(k, len(seq))
        got = deinterlace.branches(seq[a][0], seq[b][0], seq[k][0], seq[c][0], seq[d][0], seq[k][1], maxv)
        for name in total:
            total[name] += got[name]
    return total
