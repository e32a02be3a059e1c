"""Frames with bars for the content-box tests (tests/test_bars_host.py, tests/test_gpu_bars.py): numpy only, seeded."""
import numpy as np

from pfnl_amd import bars, scene


def dtype_of(maxv):
    return np.uint8 if maxv == 255 else np.uint16


def luma(frame):
    return scene.luma_u10(frame) if frame.dtype == np.uint16 else scene.luma_u8(frame)


def boxed(H, W, box, maxv=255, seed=0, noise=0):
    """random picture (luma well above any limit used) inside ``box``, bars of noise with luma at most ``noise`` around it"""
    rng = np.random.default_rng(seed + 131 * H + W)
    top = noise * (1 if maxv == 255 else 4)
    f = rng.integers(0, top + 1, (H, W, 3)).astype(dtype_of(maxv))
    y0, x0, h, w = box
    f[y0:y0 + h, x0:x0 + w] = rng.integers(maxv // 2, maxv + 1, (h, w, 3))
    return f


def cases(H, W, maxv=255, seed=0):
    """name -> frame: the picture in the middle, touching each edge, the whole frame, all black, noise below the limit in the bars"""
    qy, qx = max(H // 4, 1) if H > 2 else 0, max(W // 4, 1) if W > 2 else 0
    mid = (qy, qx, max(H - 2 * qy, 1), max(W - 2 * qx, 1))
    out = {
        "middle": boxed(H, W, mid, maxv, seed),
        "top": boxed(H, W, (0, mid[1], mid[2], mid[3]), maxv, seed + 1),
        "bottom": boxed(H, W, (H - mid[2], mid[1], mid[2], mid[3]), maxv, seed + 2),
        "left": boxed(H, W, (mid[0], 0, mid[2], mid[3]), maxv, seed + 3),
        "right": boxed(H, W, (mid[0], W - mid[3], mid[2], mid[3]), maxv, seed + 4),
        "whole": boxed(H, W, (0, 0, H, W), maxv, seed + 5),
        "black": np.zeros((H, W, 3), dtype_of(maxv)),
        "noisy": boxed(H, W, mid, maxv, seed + 6, noise=6),
        "above1023": None,
    }
    if maxv == 1023:                                                     # samples above 1023 count as 1023
        f = boxed(H, W, mid, maxv, seed + 7)
        f[mid[0], mid[1]] = 65535
        out["above1023"] = f
    else:
        del out["above1023"]
    return out


def grey_with_luma(y, maxv=255):
    """the grey level whose luma is exactly y (0 .. 219), as a sample value"""
    for v in range(maxv + 1):
        if int(luma(np.full((1, 1, 3), v, dtype_of(maxv)))[0, 0]) == y:
            return v
    raise ValueError(y)


def at_threshold(H, W, limit, maxv=255, over=False):
    """Every row sums to exactly limit * W and every column to limit * H - a flat grey of luma ``limit`` -, so nothing is picture; ``over``:
    one pixel one level of luma brighter, so exactly its row and its column are one above their thresholds"""
    f = np.full((H, W, 3), grey_with_luma(limit, maxv), dtype_of(maxv))
    if over:
        f[H // 2, W // 3] = grey_with_luma(limit + 1, maxv)
    rows, cols = bars.line_sums(f, 10 if maxv == 1023 else 8)
    assert (rows == limit * W + (np.arange(H) == H // 2) * over).all() and (cols == limit * H + (np.arange(W) == W // 3) * over).all()
    return f
