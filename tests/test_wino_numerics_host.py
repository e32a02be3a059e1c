"""The Winograd error model of tests/numerics.py, checked on the host: the tiling and the matrices against the fp64 spec, the fp32
emulation of the kernels' algorithm against alpha_wino(K) S_w on every data family and in every mode of the persistent kernel, and
mutants of the emulation that the bound must reject (test_gpu_strict_numerics.py holds the kernels to the same bound)."""
import numpy as np
import pytest

import numerics as N
from oracle import pfnl_spec

FAMILIES = ["normal", "binades", "edges", "edges1e6", "dark16", "dark20", "bright"]
ITEMS, H, W, T = 3, 10, 38, 3                   # ragged 4 x 32 workgroup tiles in both directions; mode 1 - 3: one clip of T frames


def xdata(rng, fam, shape):
    if fam == "normal":
        return rng.normal(size=shape).astype(np.float32)
    if fam == "binades":
        return N.binades(rng, shape)
    if fam.startswith("edges"):
        return N.edges(rng, shape)
    if fam == "bright":
        return N.bright(rng, shape)
    return N.dark(rng, shape, 2.0 ** -int(fam[4:]))


def wdata(rng, fam, shape):
    if fam.startswith("edges"):
        return N.edge_weights(rng, shape, big=1.0e6 if fam == "edges1e6" else 6.0e4)
    return (rng.normal(size=shape) / np.sqrt(np.prod(shape[:-1]))).astype(np.float32)


def bias(rng, fam, n):
    scale = {"dark16": 2.0 ** -18, "dark20": 2.0 ** -22, "bright": 2.0 ** 20}.get(fam, 0.1)
    b = (rng.normal(size=n) * scale).astype(np.float32)
    b[0] = 0.0
    return b


def case(mode, fam, seed=0):
    """(emulation arguments, fp64 reference, S_w, alpha_wino) of one mode of conv_wino_ws_kernel on one family."""
    rng = np.random.default_rng([seed, mode, FAMILIES.index(fam)])
    f64 = lambda a: np.asarray(a, np.float64)                                   # noqa: E731
    cout = 48 if mode == 3 else 64
    b = bias(rng, fam, cout)
    if mode in (0, 1):
        x, k = xdata(rng, fam, (ITEMS, H, W, 64)), wdata(rng, fam, (3, 3, 64, 64))
        y = pfnl_spec.conv2d_same(f64(x), f64(k), f64(b))
        if mode == 0:
            return dict(x=x, k=k, bias=b), pfnl_spec.lrelu(y), N.wino_terms(x, k, (b,)), N.alpha_wino(64, 2)
        add, res = xdata(rng, fam, (1, H, W, 64)), xdata(rng, fam, (ITEMS, H, W, 64))
        ref = pfnl_spec.lrelu(y + f64(add)) + res
        return dict(x=x, k=k, bias=b, addend=add, resid=res), ref, N.wino_terms(x, k, (b, add, res)), N.alpha_wino(64, 4)
    if mode == 2:
        x, base, res = xdata(rng, fam, (T, H, W, 64)), xdata(rng, fam, (1, H, W, 64)), xdata(rng, fam, (T, H, W, 64))
        k = wdata(rng, fam, (3, 3, 128, 64))
        rep = np.repeat(base, T, axis=0)
        cat = np.concatenate([rep, x], axis=-1)
        ref = pfnl_spec.lrelu(pfnl_spec.conv2d_same(f64(cat), f64(k), f64(b))) + res
        return dict(x=x, k=k, bias=b, base=base, base_div=T, resid=res), ref, N.wino_terms(cat, k, (b, res)), N.alpha_wino(128, 4)
    x, k = xdata(rng, fam, (2, H, W, 64 * T)), wdata(rng, fam, (3, 3, 64 * T, cout))
    ref = pfnl_spec.lrelu(pfnl_spec.conv2d_same(f64(x), f64(k), f64(b)))
    return dict(x=x, k=k, bias=b), ref, N.wino_terms(x, k, (b,)), N.alpha_wino(64 * T, 2)


def test_fp64_winograd_is_the_spec():
    """The tiling and B^T, G, A^T: the algorithm in fp64 equals conv2d_same to 1e-12 of the largest output."""
    rng = np.random.default_rng(1)
    for shape in ((ITEMS, H, W, 64), (1, 2, 2, 64), (2, 4, 6, 5)):
        x, k = rng.normal(size=shape), rng.normal(size=(3, 3, shape[-1], 7))
        ref = pfnl_spec.conv2d_same(x, k, None)
        got = N.wino_conv_f64(x, k)
        assert got.shape == ref.shape
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_emulation_meets_the_bound(mode):
    """wino_emulate_f32 (both association orders of the output transform) within alpha_wino(K) S_w of the fp64 spec."""
    for fam in FAMILIES:
        kw, ref, Sw, a = case(mode, fam)
        for per_tile in ((False, True) if mode < 2 else (False,)):
            r = N.worst_ratio(N.wino_emulate_f32(per_tile=per_tile, **kw), ref, a * Sw)
            print(f"emulation mode {mode} {'per-tile' if per_tile else 'ws':8s} {fam:8s} worst ratio {r:.3f}")
            assert r <= 1.0, (mode, fam, per_tile, r)


def test_direct_bound_cannot_be_reused():
    """The model is needed: on the edge data the emulation exceeds alpha(576) S, the bound of the direct kernels (by a factor of
    thousands: an output's error scales with its whole 4 x 4 tile, not with its nine taps)."""
    kw, ref, _, _ = case(0, "edges")
    S, _ = N.conv_terms(kw["x"], kw["k"], (kw["bias"],))
    r = N.worst_ratio(N.wino_emulate_f32(**kw), ref, N.alpha(576) * S)
    print(f"emulation against alpha(576) S on edges: {r:.3g}")
    assert r > 1.0


def test_mutants_fail_the_bound():
    """The bound bites: three wrong versions of the emulation each fail it, where the correct one passes."""
    # an absolute offset of 2^-31 on dark16 outputs.  The op tests' 2e-5 * max(1, |ref|.max()) accepts it (and a 2^-17 one).
    kw, ref, Sw, a = case(0, "dark16")
    good = N.wino_emulate_f32(**kw).astype(np.float64)
    assert N.worst_ratio(good, ref, a * Sw) <= 1.0
    off = good + 2.0 ** -31
    assert np.abs(off - ref).max() < 2e-5 * max(1.0, np.abs(ref).max())
    r = N.worst_ratio(off, ref, a * Sw)
    print(f"mutant offset 2^-31 on dark16: {r:.3g}")
    assert r > 1.0
    # the halo column right of the image is not zero-filled (it repeats the last column)
    for fam in ("normal", "bright"):
        kw, ref, Sw, a = case(0, fam)
        bad = N.wino_emulate_f32(fault="halo", **kw)
        r = N.worst_ratio(bad, ref, a * Sw)
        print(f"mutant halo {fam}: {r:.3g}")
        assert r > 1.0
        assert N.worst_ratio(bad[:, :, :W - 2], ref[:, :, :W - 2], (a * Sw)[:, :, :W - 2]) <= 1.0    # (only the last tile column)
    # the residual added before the activation
    kw, ref, Sw, a = case(1, "normal")
    r = N.worst_ratio(N.wino_emulate_f32(fault="resid_first", **kw), ref, a * Sw)
    print(f"mutant resid before act: {r:.3g}")
    assert r > 1.0
