"""The split-f16 kernels across operand magnitudes and binary16's edges (tests/numerics.py has the model and the bound).

Every fp32 op hook that runs on the f16 matrix pipe with exactly split operands, on four data families, element-wise against the
fp64 spec: |got - ref| <= alpha(K) S + beta A.  The f32-MFMA kernel of the same op runs on the same data and must meet alpha(K) S
alone (the bound is no looser than an exact fp32 FMA chain needs).  Then bit-exact scale equivariance: with zero bias,
op(2^k x) = 2^k op(x) bit for bit wherever every split operand of the op is a kernel INPUT and the split commutes with 2^k
(numerics.equivariant_scales).  The bf16 and f32 kernels must be equivariant with no precondition.  Last, one forward on dark clips.

Data families: binades (+-2^u (1 + v), u in [-30, 14], channel c scaled by 2^((c % 9) - 4)), edges (ties, just below powers of two,
subnormal hi, hi = 0, |x| to 6.5e4; weights from 1e-7 to ~1, an all-zero output channel, one weight of 6e4), dark16 / dark20
(N(0, 1) x 2^-16 / 2^-20).  The worst bound ratio per kernel and family is printed (-s)."""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import numerics as N  # noqa: E402
from oracle import pfnl_spec  # noqa: E402
from pfnl_amd import ops  # noqa: E402

FAMILIES = ["binades", "edges", "dark16", "dark20"]
EQ_KS = (-10, -7, -1, 4, 9, 13)             # a spread of numerics.equivariant_scales(unit data) = [-10, 13]


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _grid():
    """The grid of the persistent split-f16 launches (persistent_grid: the CU count rounded down to whole XCDs, at least 8)."""
    return max(8, torch.cuda.get_device_properties(0).multi_processor_count // 8 * 8)


def _xdata(rng, fam, shape, tame=1.0):
    """Activations of a family; tame < 1 scales binades / edges down where an op re-splits its own intermediate (inside 65504)."""
    if fam == "binades":
        return (N.binades(rng, shape) * np.float32(tame)).astype(np.float32)
    if fam == "edges":
        return (N.edges(rng, shape) * np.float32(tame)).astype(np.float32)
    if fam == "dark16":
        return N.dark(rng, shape, 2.0 ** -16)
    if fam == "dark20":
        return N.dark(rng, shape, 2.0 ** -20)
    raise KeyError(fam)


def _wdata(rng, fam, shape, big=6.0e4):
    """Weights: edges -> numerics.edge_weights (big=None: no 6e4 weight, for a kernel whose output feeds another split); else
    N(0, 1 / fan-in)."""
    if fam == "edges":
        if big is None:
            w = N.edge_weights(rng, shape, big=0.0) * np.float32(2.0 ** -10)
            return w.astype(np.float32)
        return N.edge_weights(rng, shape, big=big)
    fan = int(np.prod(shape[:-1]))
    return (rng.normal(size=shape) / np.sqrt(fan)).astype(np.float32)


def _bias(rng, fam, n):
    scale = {"binades": 0.1, "edges": 0.1, "dark16": 2.0 ** -18, "dark20": 2.0 ** -22}[fam]
    b = (rng.normal(size=n) * scale).astype(np.float32)
    b[0] = 0.0
    return b


def _concat(x, T):
    """[clips*T, H, W, 64] -> [clips, H, W, 64 T] (the reference's concat over frames)."""
    F, H, W, c = x.shape
    return x.reshape(F // T, T, H, W, c).transpose(0, 2, 3, 1, 4).reshape(F // T, H, W, T * c)


def _act(y, act=True):
    return pfnl_spec.lrelu(y) if act else y


def _check(kernel, fam, got, ref, bound, f32=None):
    """got within bound of ref; f32 = (output of the f32-MFMA kernel on the same data, alpha S of that op): it must meet alpha alone."""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all(), kernel
    r = N.worst_ratio(got, ref, bound)
    msg = f"bound ratio {kernel:28s} {fam:8s} {r:.3f}"
    if f32 is not None:
        r32 = N.worst_ratio(f32[0], ref, f32[1])
        msg += f"   (f32 kernel vs alpha S: {r32:.3f})"
        assert r32 <= 1.0, (kernel, fam, "f32 kernel", r32)
    print(msg)
    assert r <= 1.0, (kernel, fam, r)


def _alpha_S(x, k, extra=()):
    S, _ = N.conv_terms(x, k, extra)
    return N.alpha(k.shape[0] * k.shape[1] * k.shape[2]) * S


# ---- numerics of the model itself on this device's inputs: the split of launch_sf_from_f32 ---------------------------------------

@pytest.mark.parametrize("fam", FAMILIES + ["unit"])
def test_chain_identity_reproduces_the_host_split(fam):
    """The device split against the host model, with nothing else in the way: conv2_i's chain launch with the identity as the frame
    half's centre tap (zero base half, bias, resid; no activation) gives hi + lo' 2^-11 of its input exactly - the input split by
    launch_sf_from_f32, hi.1 on one accumulator and lo'.1 on the other, each exact, one fp32 rounding that loses nothing.  So
    out == numerics.emulate(x) element for element (a flushed binary16 subnormal, in the split or in the MFMA operands, cannot
    pass), and the split-format copy of out (sf_split4) is split_host(out) bit for bit."""
    rng = np.random.default_rng(len(fam))
    T, clips, H, W = 3, 2, 9, 38
    x = N.unit_binades(rng, (clips * T, H, W, 64)) if fam == "unit" else _xdata(rng, fam, (clips * T, H, W, 64))
    k2 = np.zeros((3, 3, 128, 64), np.float32)
    for c in range(64):
        k2[1, 1, 64 + c, c] = 1.0
    zero_b = np.zeros((clips, H, W, 64), np.float32)
    out, out_sf = ops.conv2_chain_sf0(dev(x), k2, np.zeros(64, np.float32), dev(zero_b), dev(np.zeros_like(x)), T, act=False)
    out, out_sf = out.cpu().numpy(), out_sf.cpu().numpy()
    want = N.emulate(x)
    bad = np.argwhere(out.astype(np.float64) != want)
    print(f"identity chain {fam:8s}: max |out - x| {np.abs(out.astype(np.float64) - x).max():.3g}, max |x - emulate(x)| {np.abs(want - x).max():.3g}")
    assert bad.size == 0, (fam, len(bad), x[tuple(bad[0])], out[tuple(bad[0])], want[tuple(bad[0])])
    bad = np.argwhere(out_sf != N.split_host(out))
    assert bad.size == 0, (fam, len(bad), bad[:4])


# ---- the bound, op by op -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("variant,fused", [("split16", False), ("split16", True), ("split16_sf_in", False), ("split16_sf_in", True),
                                           ("split16_sf_out", False)])
def test_conv3x3_split16_bound(variant, fused, fam):
    """conv3x3_winograd(variant = split16 | split16_sf_in | split16_sf_out), plain and fused (the split-format output is a plain-mode
    option); 3 x 10 x 38, ragged tiles."""
    rng = np.random.default_rng(_seed(variant, fused, fam))
    items, H, W = 3, 10, 38
    osf = variant == "split16_sf_out"                                   # the output is split again: it must stay inside binary16
    x = _xdata(rng, fam, (items, H, W, 64), tame=2.0 ** -10 if osf else 1.0)
    k = _wdata(rng, fam, (3, 3, 64, 64), big=None if osf else 6.0e4)
    b = _bias(rng, fam, 64)
    kw, extra = {}, [b]
    if fused:
        add, res = _xdata(rng, fam, (1, H, W, 64)), _xdata(rng, fam, (items, H, W, 64))
        kw = dict(addend=dev(add), add_div=items, resid=dev(res))
        extra += [np.repeat(add, items, 0), res]
    y = pfnl_spec.conv2d_same(x.astype(np.float64), k.astype(np.float64), b.astype(np.float64))
    if fused:
        y = y + np.repeat(add.astype(np.float64), items, 0)
    ref = _act(y) + (res if fused else 0.0)
    bound = N.conv_bound(x, k, extra)
    if osf:
        assert np.abs(ref).max() < N.F16_MAX / 4
        bound = bound + 2.0 ** -22 * np.abs(ref) + 2.0 ** -36         # the output's own split (hi + lo' 2^-11 of the value)
    got = ops.conv3x3_winograd(dev(x), k, b, act=True, variant=variant, **kw).cpu().numpy()
    direct = ops.conv2d(dev(x), k, b, act=True, **kw).cpu().numpy()
    _check(f"conv3x3 {variant}{' fused' if fused else ''}", fam, got, ref, bound, f32=(direct, _alpha_S(x, k, extra)))


def _chain_case(rng, fam, T, clips, H, W):
    F = clips * T
    x, base, res = _xdata(rng, fam, (F, H, W, 64)), _xdata(rng, fam, (clips, H, W, 64)), _xdata(rng, fam, (F, H, W, 64))
    k2 = _wdata(rng, fam, (3, 3, 128, 64))
    b = _bias(rng, fam, 64)
    return x, base, res, k2, b


def _chain_spec(x, base, res, k2, b, T, sel):
    xs = np.concatenate([x[c * T:(c + 1) * T] for c in sel])
    cat = np.concatenate([np.repeat(base[sel], T, axis=0), xs], axis=-1)
    rs = np.concatenate([res[c * T:(c + 1) * T] for c in sel])
    ref = _act(pfnl_spec.conv2d_same(cat.astype(np.float64), k2.astype(np.float64), b.astype(np.float64))) + rs
    return cat, rs, ref


def _frames(a, T, sel):
    return np.concatenate([a[c * T:(c + 1) * T] for c in sel])


def _chain_geoms():
    return ["ragged", "chains>grid"]


def _geom(name, G):
    """(T, clips, H, W, split, sel): a ragged 2-clip case, and more chains than workgroups (G + 3 clips of one 8 x 32 chain, T = 3,
    cut behind the first round: split chains) with the fp64 spec on the first clip, the last one and those around the round boundary."""
    if name == "ragged":
        return 7, 2, 10, 38, (0, 0, 0), [0, 1]
    clips = G + 3
    return 3, clips, 8, 32, (G, 3, 1), [0, G - 1, G, clips - 1]


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("geom", _chain_geoms())
def test_conv2_chain_bound(geom, fam):
    """conv2_i in one launch: conv3x3_winograd(split16_sf_chain) and conv2_chain_ex with mfma 32 and 16 (uncut), and the 32x32x16 launch
    cut into split chains on the chains > grid geometry.  f32 yardstick: the direct kernel over [base, frame] as two frames per item."""
    G = _grid()
    T, clips, H, W, split, sel = _geom(geom, G)
    rng = np.random.default_rng(_seed(geom, fam))
    x, base, res, k2, b = _chain_case(rng, fam, T, clips, H, W)
    xd, bd, rd = dev(x), dev(base), dev(res)
    outs = {"conv2 chain mfma32": ops.conv2_chain_ex(xd, k2, b, bd, rd, T, mfma=32),
            "conv2 chain mfma16": ops.conv2_chain_ex(xd, k2, b, bd, rd, T, mfma=16)}
    if geom == "ragged":
        outs["conv3x3 split16_sf_chain"] = ops.conv3x3_winograd(xd, k2, b, act=True, addend=bd, add_div=T, resid=rd, variant="split16_sf_chain")
    else:
        outs["conv2 chain split-chains"] = ops.conv2_chain_ex(xd, k2, b, bd, rd, T, split=split)
    cat, rs, ref = _chain_spec(x, base, res, k2, b, T, sel)
    bound = N.conv_bound(cat, k2, (b, rs))
    f2 = np.stack([np.repeat(base[sel], T, axis=0), _frames(x, T, sel)], axis=1).reshape(-1, H, W, 64)
    direct = ops.conv2d(dev(f2), k2, b, act=True, frames_per_item=2, addend=dev(np.zeros((len(sel) * T, H, W, 64), np.float32)),
                        resid=dev(rs)).cpu().numpy()
    f32 = (direct, _alpha_S(cat, k2, (b, rs)))
    for name, out in outs.items():
        _check(f"{name} ({geom})", fam, _frames(out.cpu().numpy(), T, sel), ref, bound, f32=f32)
        f32 = None


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("variant", ["split16", "split16_sf:10", "split16_sf:01", "split16_sf:11"])
def test_conv1x1_split16_bound(variant, fam):
    """conv10_i: conv1x1_stream(split16 | split16_sf:io), T = 7, 2 items of 9 x 38; f32 yardstick: conv1x1_stream(stream)."""
    rng = np.random.default_rng(_seed(variant, fam))
    T, items, H, W = 7, 2, 9, 38
    osf = variant.endswith("1")                                         # split-format output: inside binary16
    x = _xdata(rng, fam, (items * T, H, W, 64), tame=2.0 ** -10 if osf else 1.0)
    k = _wdata(rng, fam, (1, 1, 64 * T, 64), big=None if osf else 6.0e4)
    b = _bias(rng, fam, 64)
    xc = _concat(x, T)
    ref = _act(pfnl_spec.conv2d_same(xc.astype(np.float64), k.astype(np.float64), b.astype(np.float64)))
    bound = N.conv_bound(xc, k, (b,))
    if osf:
        assert np.abs(ref).max() < N.F16_MAX / 4
        bound = bound + 2.0 ** -22 * np.abs(ref) + 2.0 ** -36
    got = ops.conv1x1_stream(dev(x), k, b, act=True, frames_per_item=T, variant=variant).cpu().numpy()
    stream = ops.conv1x1_stream(dev(x), k, b, act=True, frames_per_item=T, variant="stream").cpu().numpy()
    _check(f"conv1x1 {variant}", fam, got, ref, bound, f32=(stream, _alpha_S(xc, k, (b,))))


def _c1c10_refs(x, k1, b1, k10, b10, T, sel):
    xs = _frames(x, T, sel).astype(np.float64)
    ref1 = _act(pfnl_spec.conv2d_same(xs, k1.astype(np.float64), b1.astype(np.float64)))
    bound1 = N.conv_bound(xs, k1, (b1,))
    assert np.abs(ref1).max() < N.F16_MAX / 4                          # inp1 is re-split for conv10_i: keep it inside binary16
    cat = _concat(ref1, T)
    refb = _act(pfnl_spec.conv2d_same(cat, k10.astype(np.float64), b10.astype(np.float64)))
    boundb = N.conv_bound(cat, k10, (b10,), xerr=_concat(bound1, T)) + 2.0 ** -22 * np.abs(refb) + 2.0 ** -36
    bound1 = bound1 + 2.0 ** -22 * np.abs(ref1) + 2.0 ** -36           # inp1 leaves in the split format
    return ref1, bound1, refb, boundb


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("geom", _chain_geoms())
def test_conv1_conv10_bound(geom, fam):
    """conv1_i + conv10_i in one launch: conv1_conv10_split16 (sf0 off and on) and conv1_conv10_split16_ex (split chains on the
    chains > grid geometry).  conv10_i re-splits inp1 inside the kernel: its bound carries inp1's bound through |k10|."""
    G = _grid()
    T, clips, H, W, split, sel = _geom(geom, G)
    rng = np.random.default_rng(_seed(geom, fam, "c1c10"))
    x = _xdata(rng, fam, (clips * T, H, W, 64), tame=2.0 ** -10)
    k1 = _wdata(rng, fam, (3, 3, 64, 64), big=None)
    k10 = _wdata(rng, fam, (1, 1, 64 * T, 64), big=None)
    b1, b10 = _bias(rng, fam, 64), _bias(rng, fam, 64)
    xd = dev(x)
    runs = {"c1c10": ops.conv1_conv10_split16(xd, k1, b1, k10, b10, T),
            "c1c10 sf0": ops.conv1_conv10_split16(xd, k1, b1, k10, b10, T, sf0=True)}
    if geom != "ragged":
        runs["c1c10_ex split-chains"] = ops.conv1_conv10_split16_ex(xd, k1, b1, k10, b10, T, split=split)
    ref1, bound1, refb, boundb = _c1c10_refs(x, k1, b1, k10, b10, T, sel)
    direct = ops.conv2d(dev(_frames(x, T, sel)), k1, b1, act=True).cpu().numpy()
    f32 = (direct, _alpha_S(_frames(x, T, sel), k1, (b1,)))
    for name, (o1, ob) in runs.items():
        _check(f"{name} inp1 ({geom})", fam, _frames(o1.cpu().numpy(), T, sel), ref1, bound1, f32=f32)
        _check(f"{name} base ({geom})", fam, ob.cpu().numpy()[sel], refb, boundb)
        f32 = None


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("geom", _chain_geoms())
def test_conv3x3_accum_bound(geom, fam):
    """convmerge1 (448 -> 48): conv3x3_accum(split16) and conv3x3_accum_split16_ex (split chains on the chains > grid geometry);
    f32 yardstick: the direct kernel over the T concatenated frames."""
    G = _grid()
    T, clips, H, W, split, sel = _geom(geom, G)
    rng = np.random.default_rng(_seed(geom, fam, "merge1"))
    cout = 48
    x = _xdata(rng, fam, (clips * T, H, W, 64))
    k = _wdata(rng, fam, (3, 3, 64 * T, cout))
    b = _bias(rng, fam, cout)
    xd = dev(x)
    runs = {"merge1 split16": ops.conv3x3_accum(xd, k, b, act=True, frames_per_clip=T, variant="split16")}
    if geom != "ragged":
        runs["merge1_ex split-chains"] = ops.conv3x3_accum_split16_ex(xd, k, b, act=True, frames_per_clip=T, split=split)[..., :cout]
    xc = _concat(_frames(x, T, sel), T)
    ref = _act(pfnl_spec.conv2d_same(xc.astype(np.float64), k.astype(np.float64), b.astype(np.float64)))
    bound = N.conv_bound(xc, k, (b,))
    direct = ops.conv2d(dev(_frames(x, T, sel)), k, b, act=True, frames_per_item=T).cpu().numpy()
    f32 = (direct, _alpha_S(xc, k, (b,)))
    for name, out in runs.items():
        _check(f"{name} ({geom})", fam, out.cpu().numpy()[sel], ref, bound, f32=f32)
        f32 = None


@pytest.mark.parametrize("fam", FAMILIES)
def test_conv_small_bound(fam):
    """The small-shape trunk kernel (conv_small.hip): conv1_i, conv10_i, conv2_i over concat([base, f]) with residual, convmerge1;
    T = 5, 2 clips of 9 x 38.  f32 yardstick: the direct kernel on conv1_i."""
    rng = np.random.default_rng(_seed(fam, "small"))
    T, clips, H, W = 5, 2, 9, 38
    F = clips * T
    x = _xdata(rng, fam, (F, H, W, 64))
    k1, b1 = _wdata(rng, fam, (3, 3, 64, 64)), _bias(rng, fam, 64)
    ref = _act(pfnl_spec.conv2d_same(x.astype(np.float64), k1.astype(np.float64), b1.astype(np.float64)))
    direct = ops.conv2d(dev(x), k1, b1, act=True).cpu().numpy()
    _check("conv_small conv1", fam, ops.conv_small(dev(x), k1, b1).cpu().numpy(), ref, N.conv_bound(x, k1, (b1,)),
           f32=(direct, _alpha_S(x, k1, (b1,))))
    k10 = _wdata(rng, fam, (1, 1, 64 * T, 64))
    xc = _concat(x, T)
    ref = _act(pfnl_spec.conv2d_same(xc.astype(np.float64), k10.astype(np.float64), b1.astype(np.float64)))
    _check("conv_small conv10", fam, ops.conv_small(dev(x), k10, b1, b_mul=T).cpu().numpy(), ref, N.conv_bound(xc, k10, (b1,)))
    base, res = _xdata(rng, fam, (clips, H, W, 64)), _xdata(rng, fam, (F, H, W, 64))
    k2 = _wdata(rng, fam, (3, 3, 128, 64))
    cat, rs, ref = _chain_spec(x, base, res, k2, b1, T, list(range(clips)))
    got = ops.conv_small(dev(x), k2, b1, a=dev(base), a_div=T, resid=dev(res)).cpu().numpy()
    _check("conv_small conv2", fam, got, ref, N.conv_bound(cat, k2, (b1, rs)))
    km, bm = _wdata(rng, fam, (3, 3, 64 * T, 48)), _bias(rng, fam, 48)
    ref = _act(pfnl_spec.conv2d_same(xc.astype(np.float64), km.astype(np.float64), bm.astype(np.float64)))
    got = ops.conv_small(dev(x), km, bm, b_mul=T).cpu().numpy()
    _check("conv_small merge1", fam, got[..., :48], ref, N.conv_bound(xc, km, (bm,)))
    assert not got[..., 48:].any()


@pytest.mark.parametrize("fam", FAMILIES)
def test_conv_small_pf_block_bound(fam):
    """The two-launch small-shape block (conv1_i -> conv10_i partials -> conv2_i over [base, inp1] + x): inp1 and base are re-split
    inside, so the bounds carry the producers' bounds through |k|; T = 7, 1 clip of 10 x 36."""
    rng = np.random.default_rng(_seed(fam, "pf_block"))
    T, clips, H, W = 7, 1, 10, 36
    x = _xdata(rng, fam, (clips * T, H, W, 64), tame=2.0 ** -10)
    k1, k10 = _wdata(rng, fam, (3, 3, 64, 64), big=None), _wdata(rng, fam, (1, 1, 64 * T, 64), big=None)
    k2 = _wdata(rng, fam, (3, 3, 128, 64))
    b1, b10, b2 = (_bias(rng, fam, 64) for _ in range(3))
    ref1, bound1, refb, boundb = _c1c10_refs(x, k1, b1, k10, b10, T, list(range(clips)))
    cat = np.concatenate([np.repeat(refb, T, axis=0), ref1], axis=-1)
    ref2 = x + _act(pfnl_spec.conv2d_same(cat, k2.astype(np.float64), b2.astype(np.float64)))
    catb = np.concatenate([np.repeat(boundb, T, axis=0), bound1], axis=-1)
    bound2 = N.conv_bound(cat, k2, (b2, x), xerr=catb)
    g1, g2 = ops.conv_small_pf_block(dev(x), k1, b1, k10, b10, k2, b2, T)
    _check("conv_small pf_block inp1", fam, g1.cpu().numpy(), ref1, bound1)
    _check("conv_small pf_block out", fam, g2.cpu().numpy(), ref2, bound2)


# ---- bit-exact scale equivariance ----------------------------------------------------------------------------------------------------

def _scaled(arrs, k):
    return [None if a is None else (a.astype(np.float64) * 2.0 ** k).astype(np.float32) for a in arrs]


def _assert_equivariant(name, run, arrs, ks, split_inputs=True):
    """run(*arrs) -> list of outputs (numpy); every output of run(*(2^k arrs)) equals 2^k times run(*arrs) bit for bit."""
    if split_inputs:
        for a in arrs:
            if a is not None:
                assert set(ks) <= set(N.equivariant_scales(a, ks)), name          # the precondition, on the host
    base = [np.asarray(o, np.float64) for o in run(*arrs)]
    for k in ks:
        got = [np.asarray(o, np.float64) for o in run(*_scaled(arrs, k))]
        for i, (g, o) in enumerate(zip(got, base)):
            want = o * 2.0 ** k
            bad = np.argwhere(g != want)
            assert bad.size == 0, (name, k, i, len(bad), g[tuple(bad[0])], want[tuple(bad[0])])
    print(f"equivariant {name:28s} k in {list(ks)}")


def _np(*ts):
    return [t.cpu().numpy() for t in ts]


@pytest.mark.parametrize("variant,fused", [("split16", False), ("split16", True), ("split16_sf_in", False), ("split16_sf_in", True),
                                           ("split16_sf_chain", True)])
def test_conv3x3_split16_equivariant(variant, fused):
    """conv3x3_winograd(split16 | split16_sf_in [plain, fused] | split16_sf_chain [conv2_i: fused by definition]).  split16_sf_out
    re-splits its output and is held to the bound only."""
    rng = np.random.default_rng(_seed(variant, fused))
    T, clips, H, W = 3, 2, 10, 38
    x = N.unit_binades(rng, (clips * T, H, W, 64))
    cin = 128 if variant == "split16_sf_chain" else 64
    k = (rng.normal(size=(3, 3, cin, 64)) / np.sqrt(9 * cin)).astype(np.float32)
    zb = np.zeros(64, np.float32)
    if not fused:
        _assert_equivariant(f"conv3x3 {variant}", lambda a: _np(ops.conv3x3_winograd(dev(a), k, zb, act=True, variant=variant)), [x], EQ_KS)
        return
    add, res = N.unit_binades(rng, (clips, H, W, 64)), N.unit_binades(rng, (clips * T, H, W, 64))
    _assert_equivariant(f"conv3x3 {variant} fused", lambda a, ad, r: _np(ops.conv3x3_winograd(
        dev(a), k, zb, act=True, addend=dev(ad), add_div=T, resid=dev(r), variant=variant)), [x, add, res], EQ_KS)


@pytest.mark.parametrize("mfma", [32, 16])
def test_conv2_chain_equivariant(mfma):
    G = _grid()
    rng = np.random.default_rng(mfma)
    for geom in (["ragged", "chains>grid"] if mfma == 32 else ["ragged"]):
        T, clips, H, W, split, _ = _geom(geom, G)
        x, base, res = (N.unit_binades(rng, s) for s in ((clips * T, H, W, 64), (clips, H, W, 64), (clips * T, H, W, 64)))
        k2 = (rng.normal(size=(3, 3, 128, 64)) / 34).astype(np.float32)
        zb = np.zeros(64, np.float32)
        _assert_equivariant(f"conv2 chain mfma{mfma} {geom}", lambda a, bs, r: _np(ops.conv2_chain_ex(
            dev(a), k2, zb, dev(bs), dev(r), T, mfma=mfma, split=split)), [x, base, res], EQ_KS)


@pytest.mark.parametrize("variant", ["split16", "split16_sf:10"])
def test_conv1x1_split16_equivariant(variant):
    """conv1x1_stream(split16 | split16_sf:10); the variants with a split-format output (sf:01, sf:11) re-split it: bound only."""
    rng = np.random.default_rng(len(variant))
    T = 7
    x = N.unit_binades(rng, (2 * T, 9, 38, 64))
    k = (rng.normal(size=(1, 1, 64 * T, 64)) / np.sqrt(64 * T)).astype(np.float32)
    _assert_equivariant(f"conv1x1 {variant}", lambda a: _np(ops.conv1x1_stream(dev(a), k, np.zeros(64, np.float32), act=True,
                                                                               frames_per_item=T, variant=variant)), [x], EQ_KS)


def test_conv3x3_accum_split16_equivariant():
    G = _grid()
    rng = np.random.default_rng(48)
    for geom in ("ragged", "chains>grid"):
        T, clips, H, W, split, _ = _geom(geom, G)
        x = N.unit_binades(rng, (clips * T, H, W, 64))
        k = (rng.normal(size=(3, 3, 64 * T, 48)) / np.sqrt(576 * T)).astype(np.float32)
        zb = np.zeros(48, np.float32)
        _assert_equivariant(f"merge1 split16 {geom}", lambda a: _np(ops.conv3x3_accum(dev(a), k, zb, frames_per_clip=T, variant="split16")),
                            [x], EQ_KS)
        _assert_equivariant(f"merge1_ex split {geom}", lambda a: _np(ops.conv3x3_accum_split16_ex(dev(a), k, zb, frames_per_clip=T,
                                                                                                split=split)), [x], EQ_KS)


def test_conv_small_equivariant():
    """conv_small (every mode: its operands are all kernel inputs).  conv1_conv10_split16 and conv_small_pf_block re-split an
    intermediate (inp1, base) inside, whose magnitude the scale moves: they are held to the bound only."""
    rng = np.random.default_rng(5)
    T, clips, H, W = 5, 2, 9, 38
    x, base, res = (N.unit_binades(rng, s) for s in ((clips * T, H, W, 64), (clips, H, W, 64), (clips * T, H, W, 64)))
    zb = np.zeros(64, np.float32)
    k1 = (rng.normal(size=(3, 3, 64, 64)) / 24).astype(np.float32)
    k10 = (rng.normal(size=(1, 1, 64 * T, 64)) / np.sqrt(64 * T)).astype(np.float32)
    k2 = (rng.normal(size=(3, 3, 128, 64)) / 34).astype(np.float32)
    _assert_equivariant("conv_small conv1", lambda a: _np(ops.conv_small(dev(a), k1, zb)), [x], EQ_KS)
    _assert_equivariant("conv_small conv10", lambda a: _np(ops.conv_small(dev(a), k10, zb, b_mul=T)), [x], EQ_KS)
    _assert_equivariant("conv_small conv2", lambda a, bs, r: _np(ops.conv_small(dev(a), k2, zb, a=dev(bs), a_div=T, resid=dev(r))),
                        [x, base, res], EQ_KS)


BF16_KS = (-60, -20, 20, 60)


def _b16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).cuda()


def _f(*ts):
    return [t.float().cpu().numpy() for t in ts]


def test_bf16_kernels_equivariant():
    """bf16 has fp32's exponent range: every bf16 trunk kernel must commute with 2^+-20 and 2^+-60 bit for bit, on N(0, 1) data with
    no precondition - a hidden binary16 step would not."""
    rng = np.random.default_rng(16)
    T, clips, H, W = 7, 2, 10, 38
    F = clips * T
    r16 = lambda s: rng.normal(size=s).astype(np.float32)                       # noqa: E731  (rounded to bf16 by _b16; exact under 2^k)
    x, base, res = r16((F, H, W, 64)), r16((clips, H, W, 64)), r16((F, H, W, 64))
    x, base, res = (torch.from_numpy(a).to(torch.bfloat16).float().numpy() for a in (x, base, res))
    k = (rng.normal(size=(3, 3, 64, 64)) / 24).astype(np.float32)
    k10 = (rng.normal(size=(1, 1, 64 * T, 64)) / np.sqrt(64 * T)).astype(np.float32)
    km = (rng.normal(size=(3, 3, 64 * T, 48)) / np.sqrt(576 * T)).astype(np.float32)
    zb = np.zeros(64, np.float32)
    _assert_equivariant("conv3x3_bf16", lambda a: _f(ops.conv3x3_bf16(_b16(a), k, zb, act=True)), [x], BF16_KS, split_inputs=False)
    _assert_equivariant("conv3x3_bf16 fused", lambda a, bs, r: _f(ops.conv3x3_bf16(_b16(a), k, zb, act=True, addend=_b16(bs), add_div=T,
                                                                                   resid=_b16(r))), [x, base, res], BF16_KS, split_inputs=False)
    for mfma in (32, 16):
        _assert_equivariant(f"conv3x3_bf16_ex mfma{mfma}", lambda a, bs, r: _f(ops.conv3x3_bf16_ex(_b16(a), k, zb, _b16(bs), T, _b16(r),
                                                                                                  mfma=mfma)), [x, base, res], BF16_KS, split_inputs=False)
    _assert_equivariant("conv1x1_bf16", lambda a: _f(ops.conv1x1_bf16(_b16(a), k10, zb, act=True, frames_per_item=T)), [x], BF16_KS,
                        split_inputs=False)
    _assert_equivariant("conv1_conv10_bf16", lambda a: _f(*ops.conv1_conv10_bf16(_b16(a), k, zb, k10, zb, T)), [x], BF16_KS, split_inputs=False)
    _assert_equivariant("conv3x3_accum_bf16", lambda a: _f(ops.conv3x3_accum_bf16(_b16(a), km, zb[:48], act=True, frames_per_clip=T)), [x],
                        BF16_KS, split_inputs=False)


def test_f32_kernels_equivariant():
    """The f32-MFMA kernels (direct, Winograd, persistent Winograd in its four modes, 1x1 stream): bit-equivariant under 2^+-40."""
    rng = np.random.default_rng(32)
    T, items, H, W = 7, 2, 10, 38
    x = rng.normal(size=(items * T, H, W, 64)).astype(np.float32)
    add, res = rng.normal(size=(items, H, W, 64)).astype(np.float32), rng.normal(size=(items * T, H, W, 64)).astype(np.float32)
    k = (rng.normal(size=(3, 3, 64, 64)) / 24).astype(np.float32)
    k10 = (rng.normal(size=(1, 1, 64 * T, 64)) / np.sqrt(64 * T)).astype(np.float32)
    zb = np.zeros(64, np.float32)
    ks = (-40, 40)
    _assert_equivariant("conv2d direct fused", lambda a, ad, r: _np(ops.conv2d(dev(a), k, zb, act=True, addend=dev(ad), add_div=T,
                                                                               resid=dev(r))), [x, add, res], ks, split_inputs=False)
    for v in ("winograd", "winograd_ws"):
        _assert_equivariant(f"conv3x3 {v} fused", lambda a, ad, r: _np(ops.conv3x3_winograd(dev(a), k, zb, act=True, addend=dev(ad), add_div=T,
                                                                                           resid=dev(r), variant=v)), [x, add, res], ks, split_inputs=False)
    _assert_equivariant("conv1x1 stream", lambda a: _np(ops.conv1x1_stream(dev(a), k10, zb, act=True, frames_per_item=T)), [x], ks,
                        split_inputs=False)
    k2 = (rng.normal(size=(3, 3, 128, 64)) / 34).astype(np.float32)
    _assert_equivariant("conv2_grouped (ws mode 2)", lambda a, ad, r: _np(ops.conv2_grouped(dev(a), dev(ad), k2, zb, dev(r), T)), [x, add, res], ks,
                        split_inputs=False)
    for cout in (48, 64):
        km = (rng.normal(size=(3, 3, 64 * T, cout)) / np.sqrt(576 * T)).astype(np.float32)
        _assert_equivariant(f"conv3x3_accum winograd (ws mode 3) cout {cout}", lambda a: _np(ops.conv3x3_accum(
            dev(a), km, zb[:cout], act=True, frames_per_clip=T, variant="winograd")), [x], ks, split_inputs=False)


# ---- one forward on dark clips -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [12, 20])
@pytest.mark.parametrize("biases", ["synthetic", "zero"])
def test_forward_dark_clips(dim, biases):
    """uniform_clips x 2^-dim through the whole forward (num_block 2), default path and strict_fp32=on, against the fp64 spec.  With
    zero biases the trunk's activations stay dark as well.  The default path's worst error is at most 2x the strict path's plus the
    operand floor of its split convolutions: beta times the largest sum |k| of an output channel, summed over the network's
    convolutions (the weight operands' share of A when every activation sits under 2^-12).  Neither run may leave binary16's
    range (no re-run on the f32 kernels)."""
    from pfnl_amd import synth
    from pfnl_amd.engine import PFNLEngine
    from pfnl_amd.spec import PFNLGeometry
    geom = PFNLGeometry(num_block=2)
    w = synth.synthetic_weights(geom, seed=3)
    if biases == "zero":
        w = {n: (np.zeros_like(a) if n.endswith("/bias") else a) for n, a in w.items()}
    x = (synth.uniform_clips(1, 7, 16, 24, seed=7) * np.float32(2.0 ** -dim)).astype(np.float32)
    ref = pfnl_spec.forward(x.astype(np.float64), w, num_block=2)
    errs = {}
    for mode in ("default", "strict"):
        eng = PFNLEngine(geom, device=0)
        eng.load_weights(w)
        if mode == "strict":
            eng.set_option("strict_fp32", "on")
        y = eng.forward(x)
        assert eng.range_reruns() == 0, mode
        errs[mode] = float(np.abs(y.astype(np.float64) - ref).max())
    kern = [np.abs(a.astype(np.float64)).reshape(-1, a.shape[-1]).sum(0).max() for n, a in w.items() if n.endswith("/kernel")]
    floor = N.BETA * float(np.sum(kern))
    print(f"forward dark 2^-{dim} biases={biases}: max|ref| {np.abs(ref).max():.3g}, err default {errs['default']:.3g}, "
          f"strict {errs['strict']:.3g}, floor {floor:.3g}")
    assert errs["default"] <= 2.0 * errs["strict"] + floor, (errs, floor)
