"""The strict-fp32 kernels across operand magnitudes, element-wise against the fp64 spec (tests/numerics.py has the models).

The strict set - the per-tile and the persistent Winograd F(2x2,3x3) kernels (modes 0 - 3), the direct f32-MFMA kernel, the 1x1 stream
kernel, the VALU conv0 and the tail - runs when strict_fp32=on, when a weight lies beyond binary16 and when a forward's activations
left binary16's range: on values of 1e5 and beyond and on mixed magnitudes.  Here every kernel of the set meets its bound on such
data, element by element:

  - the Winograd kernels: |got - ref| <= alpha_wino(K) S_w, and the rms of err / S_w is at most 1.5 times that of
    numerics.wino_emulate_f32 (the plain fp32 statement of the same algorithm) on the same data: the project's standing criterion
    e_s <= 1.5 e_d of test_gpu_ops.py with the emulation in the other kernel's place;
  - the direct, 1x1 stream, VALU conv0 and tail kernels: alpha(K) S (the tail: plus its bicubic term); the split-f16 conv0 kernel:
    alpha(75) S + beta A, as the other split-f16 kernels in test_gpu_numerics.py.

Every call is made twice and must repeat bit for bit.  Geometries: 3 items of 10 x 38 (ragged 4 x 32 workgroup tiles in both directions,
halo on every side), 2 x 2 (everything is halo) and 12 x 64 items, six tiles each, more (item, tile) units than the persistent kernel
has workgroups, with the spec on the first and last item and those where a workgroup goes from its first unit to its second.
Families: binades, edges (x to 6.5e4; weights 1e-7 .. 1, one of 1e6: beyond binary16), dark16, bright (+-2^[10, 40]).  The worst
bound ratio and the rms ratio per kernel and family are printed (-s)."""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import numerics as N  # noqa: E402
from oracle import pfnl_spec  # noqa: E402
from pfnl_amd import ops  # noqa: E402

FAMILIES = ["binades", "edges", "dark16", "bright"]
WS_MAX_WORKGROUPS = 256                         # conv_wino_ws.hip: 8 XCDs x min(rs, 32) workgroups


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _f64(a):
    return np.asarray(a, np.float64)


def _xdata(rng, fam, shape):
    if fam == "binades":
        return N.binades(rng, shape)
    if fam == "edges":
        return N.edges(rng, shape)
    if fam == "bright":
        return N.bright(rng, shape)
    if fam == "normal":
        return rng.normal(size=shape).astype(np.float32)
    return N.dark(rng, shape, 2.0 ** -int(fam[4:]))


def _wdata(rng, fam, shape, big=1.0e6):
    if fam == "edges":
        return N.edge_weights(rng, shape, big=big)
    return (rng.normal(size=shape) / np.sqrt(np.prod(shape[:-1]))).astype(np.float32)


def _bias(rng, fam, n):
    scale = {"dark16": 2.0 ** -18, "dark20": 2.0 ** -22, "bright": 2.0 ** 20}.get(fam, 0.1)
    b = (rng.normal(size=n) * scale).astype(np.float32)
    b[0] = 0.0
    return b


def _twice(run):
    """The op's output (numpy); a second call must give the same bits."""
    a, b = run().cpu().numpy(), run().cpu().numpy()
    assert np.array_equal(a.view(np.int32), b.view(np.int32)), "the call does not repeat bit for bit"
    return a


def _check(kernel, fam, got, ref, bound):
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all(), kernel
    r = N.worst_ratio(got, ref, bound)
    print(f"bound ratio {kernel:44s} {fam:8s} {r:.3f}")
    assert r <= 1.0, (kernel, fam, r)


def _rms(got, ref, Sw):
    m = Sw > 0
    return float(np.sqrt(np.mean(((np.asarray(got, np.float64) - ref)[m] / Sw[m]) ** 2)))


def _check_wino(kernel, fam, got, ref, Sw, a, emu):
    """The bound, then sharpness: rms(err / S_w) of the kernel at most 1.5 times the emulation's (which must meet the bound too)."""
    assert N.worst_ratio(emu, ref, a * Sw) <= 1.0, (kernel, fam, "the emulation misses the bound: the derivation is wrong")
    _check(kernel, fam, got, ref, a * Sw)
    ek, ee = _rms(got, ref, Sw), _rms(emu, ref, Sw)
    print(f"rms ratio   {kernel:44s} {fam:8s} {ek / ee:.3f}   (kernel {ek:.3g}, emulation {ee:.3g})")
    assert ek <= 1.5 * ee, (kernel, fam, ek, ee)


# ---- geometries -----------------------------------------------------------------------------------------------------------------------

def _ws_limit():
    """Workgroups the persistent Winograd launch can have: 8 XCDs x min(rs, 32).  Never under the CU count rounded down to whole XCDs
    (the grid of the persistent split-f16 launches), so the chained geometry chains on any device."""
    return max(WS_MAX_WORKGROUPS, torch.cuda.get_device_properties(0).multi_processor_count // 8 * 8)


def _geometry(name, T=1):
    """(groups, H, W, selected groups): a group is an item (modes 0, 1; a multiple of T of them) or a clip (modes 2, 3).  `chained`:
    12 x 64 = six 4 x 32 tiles per group and more tiles than workgroups; XCD x owns tiles [x rs, x rs + rs), its workgroup j takes
    j, j + 32, ...: the spec on the groups of tiles 0, 31 | 32 (XCD 0's round boundary), rs + 31 | rs + 32 (XCD 1's) and the last."""
    if name == "ragged":
        return 3 if T == 1 else T, 10, 38, None
    if name == "2x2":
        return 3 if T == 1 else T, 2, 2, None
    per = 6
    groups = _ws_limit() // per + 3
    groups += -groups % T
    ntiles = groups * per
    rs = (ntiles + 7) // 8
    assert rs > 32 and ntiles > _ws_limit()
    return groups, 12, 64, [0, 31, 32, rs + 31, rs + 32, ntiles - 1]


def _items_of_tiles(tiles, per, grp, n):
    """Items the tiles of a plain / fused launch belong to (conv_wino_ws.hip, WS_UNIT: with grp = add_div > 1 the grp frames of a clip at
    one spatial tile are consecutive units)."""
    out = []
    for t in tiles:
        c, r = divmod(t, per * grp)
        out.append(c * grp + r % grp)
    return sorted(set(i for i in out if i < n))


def _clips_of_tiles(tiles):
    """Clips of a grouped / accumulating launch (units = (clip, tile) groups, clip-major): those of the first tile, XCD 0's round
    boundary and the last tile."""
    return sorted(set(t // 6 for t in (tiles[0], tiles[1], tiles[2], tiles[-1])))


GEOMS = ["ragged", "2x2", "chained"]


# ---- modes 0 and 1: conv1_i and the halves of conv2_i ---------------------------------------------------------------------------------

@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("variant", ["winograd", "winograd_ws"])
def test_conv3x3_winograd_bound(variant, fused, geom, fam):
    """ops.conv3x3_winograd(winograd | winograd_ws), plain (mode 0) and fused (mode 1: addend at add_div = T, resid); K = 64."""
    T = 3
    rng = np.random.default_rng(_seed(variant, fused, geom, fam))
    items, H, W, tiles = _geometry(geom, T if fused else 1)
    x, k, b = _xdata(rng, fam, (items, H, W, 64)), _wdata(rng, fam, (3, 3, 64, 64)), _bias(rng, fam, 64)
    sel = list(range(items)) if tiles is None else _items_of_tiles(tiles, 6, T if fused else 1, items)
    kw, ekw, extra = {}, {}, [b]
    if fused:
        add, res = _xdata(rng, fam, (items // T, H, W, 64)), _xdata(rng, fam, (items, H, W, 64))
        kw = dict(addend=dev(add), add_div=T, resid=dev(res))
        adds = add[[i // T for i in sel]]
        ekw = dict(addend=adds, resid=res[sel])
        extra += [adds, res[sel]]
    got = _twice(lambda: ops.conv3x3_winograd(dev(x), k, b, act=True, variant=variant, **kw))[sel]
    xs = x[sel]
    y = pfnl_spec.conv2d_same(_f64(xs), _f64(k), _f64(b))
    ref = pfnl_spec.lrelu(y + _f64(ekw["addend"])) + _f64(ekw["resid"]) if fused else pfnl_spec.lrelu(y)
    emu = N.wino_emulate_f32(xs, k, b, per_tile=variant == "winograd", **ekw)
    _check_wino(f"conv3x3 {variant}{' fused' if fused else ''} ({geom})", fam, got, ref, N.wino_terms(xs, k, extra),
                N.alpha_wino(64, 4 if fused else 2), emu)


# ---- mode 2: conv2_i in one launch ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fam", ["normal"] + FAMILIES)
@pytest.mark.parametrize("geom,T", [("ragged", 3), ("ragged", 7), ("2x2", 3), ("chained", 3)])
def test_conv2_grouped_bound(geom, T, fam):
    """ops.conv2_grouped: the base half's raw result stays in LDS and joins every frame's epilogue; K = 128."""
    rng = np.random.default_rng(_seed(geom, T, fam, "grouped"))
    clips, H, W, tiles = _geometry(geom)
    clips = 2 if tiles is None else clips
    x, base, res = (_xdata(rng, fam, s) for s in ((clips * T, H, W, 64), (clips, H, W, 64), (clips * T, H, W, 64)))
    k, b = _wdata(rng, fam, (3, 3, 128, 64)), _bias(rng, fam, 64)
    sel = list(range(clips)) if tiles is None else _clips_of_tiles(tiles)
    got = _twice(lambda: ops.conv2_grouped(dev(x), dev(base), k, b, dev(res), T))
    fr = np.concatenate([np.arange(c * T, (c + 1) * T) for c in sel])
    rep = np.repeat(base[sel], T, axis=0)
    cat = np.concatenate([rep, x[fr]], axis=-1)
    ref = pfnl_spec.lrelu(pfnl_spec.conv2d_same(_f64(cat), _f64(k), _f64(b))) + res[fr]
    emu = N.wino_emulate_f32(x[fr], k, b, base=base[sel], base_div=T, resid=res[fr])
    _check_wino(f"conv2_grouped T={T} ({geom})", fam, got[fr], ref, N.wino_terms(cat, k, (b, res[fr])), N.alpha_wino(128, 4), emu)


# ---- mode 3: convmerge1 ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("geom,T,cout", [("ragged", 3, 48), ("ragged", 3, 64), ("ragged", 7, 48), ("ragged", 7, 64), ("2x2", 3, 48),
                                         ("chained", 3, 48)])
def test_conv3x3_accum_winograd_bound(geom, T, cout, fam):
    """ops.conv3x3_accum(variant="winograd"): the T frames of a clip into one set of accumulators; K = 64 T."""
    rng = np.random.default_rng(_seed(geom, T, cout, fam, "accum"))
    clips, H, W, tiles = _geometry(geom)
    clips = 2 if tiles is None else clips
    x = _xdata(rng, fam, (clips * T, H, W, 64))
    k, b = _wdata(rng, fam, (3, 3, 64 * T, cout)), _bias(rng, fam, cout)
    sel = list(range(clips)) if tiles is None else _clips_of_tiles(tiles)
    got = _twice(lambda: ops.conv3x3_accum(dev(x), k, b, act=True, frames_per_clip=T, variant="winograd"))[sel]
    xc = x.reshape(clips, T, H, W, 64)[sel].transpose(0, 2, 3, 1, 4).reshape(len(sel), H, W, 64 * T)
    ref = pfnl_spec.lrelu(pfnl_spec.conv2d_same(_f64(xc), _f64(k), _f64(b)))
    emu = N.wino_emulate_f32(xc, k, b)
    _check_wino(f"conv3x3_accum winograd T={T} cout={cout} ({geom})", fam, got, ref, N.wino_terms(xc, k, (b,)), N.alpha_wino(64 * T, 2), emu)


# ---- the direct and the 1x1 stream kernel beyond binary16 (the yardsticks of test_gpu_numerics.py on the other families) ---------------

@pytest.mark.parametrize("fused", [False, True])
def test_conv2d_direct_bright(fused):
    rng = np.random.default_rng(_seed("direct", fused))
    items, H, W, fam = 3, 10, 38, "bright"
    x, k, b = _xdata(rng, fam, (items, H, W, 64)), _wdata(rng, fam, (3, 3, 64, 64)), _bias(rng, fam, 64)
    y = pfnl_spec.conv2d_same(_f64(x), _f64(k), _f64(b))
    kw, extra = {}, [b]
    if fused:
        add, res = _xdata(rng, fam, (1, H, W, 64)), _xdata(rng, fam, (items, H, W, 64))
        kw = dict(addend=dev(add), add_div=items, resid=dev(res))
        extra += [add, res]
        y = y + _f64(add)
    ref = pfnl_spec.lrelu(y) + (_f64(res) if fused else 0.0)
    S, _ = N.conv_terms(x, k, extra)
    got = _twice(lambda: ops.conv2d(dev(x), k, b, act=True, **kw))
    _check(f"conv2d direct{' fused' if fused else ''}", fam, got, ref, N.alpha(576) * S)


@pytest.mark.parametrize("T", [3, 7])
def test_conv1x1_stream_bright(T):
    rng = np.random.default_rng(_seed("stream", T))
    items, H, W, fam = 2, 9, 38, "bright"
    x, k, b = _xdata(rng, fam, (items * T, H, W, 64)), _wdata(rng, fam, (1, 1, 64 * T, 64)), _bias(rng, fam, 64)
    xc = x.reshape(items, T, H, W, 64).transpose(0, 2, 3, 1, 4).reshape(items, H, W, 64 * T)
    ref = pfnl_spec.lrelu(pfnl_spec.conv2d_same(_f64(xc), _f64(k), _f64(b)))
    S, _ = N.conv_terms(xc, k, (b,))
    got = _twice(lambda: ops.conv1x1_stream(dev(x), k, b, act=True, frames_per_item=T, variant="stream"))
    _check(f"conv1x1 stream T={T}", fam, got, ref, N.alpha(64 * T) * S)


# ---- conv0: the split-f16 MFMA kernel and the VALU kernel of strict mode -------------------------------------------------------------------

@pytest.mark.parametrize("fam", ["binades", "edges", "dark16", "dark20", "bright"])
@pytest.mark.parametrize("B,T,H,W", [(1, 3, 10, 38), (1, 7, 2, 2)])
def test_conv0_bound(B, T, H, W, fam):
    """ops.conv0: the default kernel (conv0_mfma_kernel, split-f16: alpha(75) S + beta A, inside binary16 only) and f32=True
    (conv0_kernel, an fp32 FMA chain of 75 products from the bias: alpha(75) S, on bright as well)."""
    rng = np.random.default_rng(_seed("conv0", T, H, W, fam))
    x = _xdata(rng, fam, (B, T, H, W, 3))
    k, b = _wdata(rng, fam, (5, 5, 3, 64), big=6.0e4), _bias(rng, fam, 64)
    xf = x.reshape(B * T, H, W, 3)
    ref = pfnl_spec.lrelu(pfnl_spec.conv2d_same(_f64(xf), _f64(k), _f64(b)))
    S, _ = N.conv_terms(xf, k, (b,))
    got = _twice(lambda: ops.conv0(dev(x), k, b, f32=True))
    _check(f"conv0 f32 (VALU) T={T} {H}x{W}", fam, got, ref, N.alpha(75) * S)
    if fam != "bright":
        got = _twice(lambda: ops.conv0(dev(x), k, b))
        _check(f"conv0 default (split-f16) T={T} {H}x{W}", fam, got, ref, N.conv_bound(xf, k, (b,)))


# ---- the tail -------------------------------------------------------------------------------------------------------------------------

def _bicubic_abs(x, scale):
    """sum |w_tap| |x| of pfnl_spec.resize_bicubic_tf1 (the same taps and clamped indices, magnitudes instead of values)."""
    x = np.abs(_f64(x))
    B, H, W, C = x.shape

    def tables(n_in):
        idx = np.array([np.clip(np.arange(o // scale - 1, o // scale + 3), 0, n_in - 1) for o in range(n_in * scale)])
        wts = np.array([np.abs(pfnl_spec._bicubic_taps((o % scale) / scale)) for o in range(n_in * scale)])
        return idx, wts

    (iy, wy), (ix, wx) = tables(H), tables(W)
    tmp = sum(x[:, :, ix[:, t], :] * wx[None, None, :, t, None] for t in range(4))
    return sum(tmp[:, iy[:, t], :, :] * wy[None, :, t, None, None] for t in range(4))


@pytest.mark.parametrize("fam", ["binades", "dark16"])
@pytest.mark.parametrize("B,T,H,W,scale", [(2, 3, 5, 19, 4), (2, 5, 6, 20, 2), (1, 7, 1, 1, 4)])
def test_tail_bound(B, T, H, W, scale, fam):
    """ops.tail: convmerge2 is an fp32 FMA chain of 108 products from the bias (alpha(108) S); the bicubic is two chains of four FMAs
    from zero (exact tap weights at quarters and halves): 8 roundings, each at most 2^-24 of sum |w_tap| |x|, and the final
    conv + bicubic addition one more: 2^-24 9 sum |w_tap| |x| (the addition's share of S lies inside alpha's 2^-22)."""
    rng = np.random.default_rng(_seed("tail", H, W, scale, fam))
    merge, x = _xdata(rng, fam, (B, H, W, 48)), _xdata(rng, fam, (B, T, H, W, 3))
    co = 12 if scale == 4 else 3
    k, b = _wdata(rng, fam, (3, 3, 12, co)), _bias(rng, fam, co)
    large = pfnl_spec.depth_to_space2(_f64(merge))
    o = pfnl_spec.conv2d_same(large, _f64(k), _f64(b))
    S, _ = N.conv_terms(large, k, (b,))
    if scale == 4:
        o, S = pfnl_spec.depth_to_space2(o), pfnl_spec.depth_to_space2(S)
    xc = x[:, T // 2]
    ref = (o + pfnl_spec.resize_bicubic_tf1(_f64(xc), scale))[:, None]
    bound = (N.alpha(108) * S + 2.0 ** -24 * 9 * _bicubic_abs(xc, scale))[:, None]
    got = _twice(lambda: ops.tail(dev(merge), dev(x), k, b, scale))
    _check(f"tail x{scale} {H}x{W}", fam, got, ref, bound)
