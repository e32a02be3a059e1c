"""conv1_i's 3x3 stage of the fused conv1_i + conv10_i launch on v_mfma_f32_16x16x32_f16 (conv3x3_c1c10_kernel<., ., M16>; reference
model/pfnl.py:66-68): the op hook pfnl_op_conv1_conv10_split16_mfma against the fp64 spec and against the 32x32x16 kernel,
its weight pack by exact answers, the operand-magnitude families of tests/numerics.py, and the forward under the default option."""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import numerics as N  # noqa: E402
from oracle import pfnl_fast, pfnl_spec  # noqa: E402
from pfnl_amd import ops, synth  # noqa: E402
from pfnl_amd.engine import PFNLEngine  # noqa: E402
from pfnl_amd.spec import PFNLGeometry  # noqa: E402

ABS_TOL = 5e-5              # the forward's element-wise bound of test_gpu_forward.py


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _grid():
    return max(8, torch.cuda.get_device_properties(0).multi_processor_count // 8 * 8)


@pytest.mark.parametrize("T,clips,H,W", [(7, 1, 8, 32), (7, 2, 16, 64), (5, 1, 9, 38), (3, 3, 5, 7), (7, 1, 1, 1), (7, 1, 33, 70),
                                          (7, 4, 128, 128), (5, 2, 64, 96), (1, 2, 24, 40), (7, 40, 8, 32)])
def test_conv1_conv10_mfma16(T, clips, H, W):
    """The geometries and bounds of test_conv1_conv10_fused_split16: inp1 and base against the fp64 spec (4e-6 max(1, |ref|max)), the error no
    more than 1.5 x the 32x32x16 kernel's on the same input (the standing criterion for a split-f16 kernel), every call repeated bit for bit."""
    rng = np.random.default_rng(T * 1000 + H * 10 + W + clips)
    F = clips * T
    x = rng.normal(size=(F, H, W, 64)).astype(np.float32)
    k1 = (rng.normal(size=(3, 3, 64, 64)) / 24.0).astype(np.float32)
    b1 = (rng.normal(size=64) * 0.1).astype(np.float32)
    k10 = (rng.normal(size=(1, 1, 64 * T, 64)) / np.sqrt(64 * T)).astype(np.float32)
    b10 = (rng.normal(size=64) * 0.1).astype(np.float32)
    xd = dev(x)
    got1, gotb = (t.cpu().numpy() for t in ops.conv1_conv10_split16_mfma(xd, k1, b1, k10, b10, T, mfma=16))
    for rep in range(2):
        r1, rb = (t.cpu().numpy() for t in ops.conv1_conv10_split16_mfma(xd, k1, b1, k10, b10, T, mfma=16))
        assert np.array_equal(r1.view(np.uint32), got1.view(np.uint32)) and np.array_equal(rb.view(np.uint32), gotb.view(np.uint32)), rep
    old1, oldb = (t.cpu().numpy() for t in ops.conv1_conv10_split16_mfma(xd, k1, b1, k10, b10, T, mfma=32))
    ref32 = [t.cpu().numpy() for t in ops.conv1_conv10_split16(xd, k1, b1, k10, b10, T)]
    assert np.array_equal(old1.view(np.uint32), ref32[0].view(np.uint32)) and np.array_equal(oldb.view(np.uint32), ref32[1].view(np.uint32))
    big = F * H * W > 200000                                                        # fp64 spec on a subset of the clips only
    nc = 1 if big else clips
    ref1 = pfnl_spec.lrelu(pfnl_spec.conv2d_same(x[:nc * T].astype(np.float64), k1.astype(np.float64), b1.astype(np.float64)))
    cat = ref1.reshape(nc, T, H, W, 64).transpose(0, 2, 3, 1, 4).reshape(nc, H, W, T * 64)
    refb = pfnl_spec.lrelu(pfnl_spec.conv2d_same(cat, k10.astype(np.float64), b10.astype(np.float64)))
    e1, eb = np.abs(got1[:nc * T] - ref1).max(), np.abs(gotb[:nc] - refb).max()
    o1, ob = np.abs(old1[:nc * T] - ref1).max(), np.abs(oldb[:nc] - refb).max()
    print(f"c1c10 mfma16 T{T} {clips}x{H}x{W}: inp1 err {e1:.3g} (32x32x16: {o1:.3g}), base err {eb:.3g} ({ob:.3g}), "
          f"max |16 - 32| inp1 {np.abs(got1 - old1).max():.3g} base {np.abs(gotb - oldb).max():.3g}")
    assert e1 < 4e-6 * max(1.0, np.abs(ref1).max()) and eb < 4e-6 * max(1.0, np.abs(refb).max()), (e1, eb)
    assert e1 <= 1.5 * o1 and eb <= 1.5 * ob, (e1, o1, eb, ob)


def _exact_taps():
    """One one-hot tap (ky, kx, ci) per output channel: every 16-channel output tile sees the 9 taps; ci(co) = (37 co + 5) mod 64 is a
    permutation of the input channels (both channel halves, every 8-channel chunk)."""
    return [(((co * 5 + co // 9) % 9) // 3, ((co * 5 + co // 9) % 9) % 3, (37 * co + 5) % 64) for co in range(64)]


@pytest.mark.parametrize("mfma", [16, 32])
@pytest.mark.parametrize("T,clips,H,W", [(3, 2, 11, 45), (7, 1, 9, 70), (5, 1, 1, 1)])
def test_c1c10_pack_orders_exact(T, clips, H, W, mfma):
    """Exact answers that pin every entry of conv3x3_split16_pack_weights16(perm_rows) (and of the 32x32x16 pack beside it): one one-hot tap of
    weight 2^k per output channel and inputs that are small positive integers, so inp1 is the zero-padded shifted input times a power of two
    and base (one-hot conv10_i: frame f(co), channel c(co)) that times another - every value exact in binary16, lo' = 0, leaky-relu the
    identity.  A transposed or permuted output tile puts a channel's values somewhere else: caught bit for bit."""
    g = torch.Generator().manual_seed(T * 10 + H)
    taps = _exact_taps()
    wval = np.exp2(torch.randint(-3, 3, (64,), generator=g).float().numpy()).astype(np.float32)
    k = np.zeros((3, 3, 64, 64), np.float32)
    for co, (ky, kx, ci) in enumerate(taps):
        k[ky, kx, ci, co] = wval[co]
    Fr = clips * T
    x = torch.randint(1, 64, (Fr, H, W, 64), generator=g).float()
    k10 = np.zeros((1, 1, 64 * T, 64), np.float32)
    w10 = np.exp2(torch.randint(-2, 2, (64,), generator=g).float().numpy()).astype(np.float32)
    for co in range(64):
        k10[0, 0, (co % T) * 64 + (29 * co + 3) % 64, co] = w10[co]
    out1, base = ops.conv1_conv10_split16_mfma(x.cuda(), k, np.zeros(64, np.float32), k10, np.zeros(64, np.float32), T, mfma=mfma)
    pad = torch.zeros(Fr, H + 2, W + 2, 64)
    pad[:, 1:H + 1, 1:W + 1] = x
    want1 = torch.zeros(Fr, H, W, 64)
    for co, (ky, kx, ci) in enumerate(taps):
        want1[..., co] = pad[:, ky:ky + H, kx:kx + W, ci] * float(wval[co])
    assert torch.equal(out1.cpu(), want1), int((out1.cpu() != want1).sum())
    w1 = want1.reshape(clips, T, H, W, 64)
    wantb = torch.stack([w1[:, co % T, :, :, (29 * co + 3) % 64] * float(w10[co]) for co in range(64)], dim=-1)
    assert torch.equal(base.cpu(), wantb), int((base.cpu() != wantb).sum())


# ---- operand magnitudes and binary16 edges: the families and the bound function test_gpu_numerics.py runs on the 32x32x16 op -------------
FAMILIES = ["binades", "edges", "dark16", "dark20"]


def _xdata(rng, fam, shape, tame=1.0):
    if fam == "binades":
        return (N.binades(rng, shape) * np.float32(tame)).astype(np.float32)
    if fam == "edges":
        return (N.edges(rng, shape) * np.float32(tame)).astype(np.float32)
    return N.dark(rng, shape, 2.0 ** -16 if fam == "dark16" else 2.0 ** -20)


def _wdata(rng, fam, shape):
    if fam == "edges":
        return (N.edge_weights(rng, shape, big=0.0) * np.float32(2.0 ** -10)).astype(np.float32)
    return (rng.normal(size=shape) / np.sqrt(int(np.prod(shape[:-1])))).astype(np.float32)


def _bias(rng, fam, n):
    b = (rng.normal(size=n) * {"binades": 0.1, "edges": 0.1, "dark16": 2.0 ** -18, "dark20": 2.0 ** -22}[fam]).astype(np.float32)
    b[0] = 0.0
    return b


def _concat(x, T):
    F, H, W, c = x.shape
    return x.reshape(F // T, T, H, W, c).transpose(0, 2, 3, 1, 4).reshape(F // T, H, W, T * c)


def _frames(a, T, sel):
    return np.concatenate([a[c * T:(c + 1) * T] for c in sel])


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("geom", ["ragged", "chains>grid"])
def test_c1c10_mfma16_bound(geom, fam):
    """test_conv1_conv10_bound's data, geometries and bound (|got - ref| <= alpha(K) S + beta A element-wise against the fp64 spec; conv10_i's
    bound carries inp1's through |k10|) on the 16x16x32 form.  chains > grid: G + 3 clips of one 8 x 32 chain, dealt out whole (the form has no
    split chains), the spec on the first clip, the last one and those around the round boundary."""
    G = _grid()
    T, clips, H, W, sel = (7, 2, 10, 38, [0, 1]) if geom == "ragged" else (3, G + 3, 8, 32, [0, G - 1, G, G + 2])
    rng = np.random.default_rng(zlib.crc32(repr((geom, fam, "c1c10")).encode()))
    x = _xdata(rng, fam, (clips * T, H, W, 64), tame=2.0 ** -10)
    k1 = _wdata(rng, fam, (3, 3, 64, 64))
    k10 = _wdata(rng, fam, (1, 1, 64 * T, 64))
    b1, b10 = _bias(rng, fam, 64), _bias(rng, fam, 64)
    o1, ob = ops.conv1_conv10_split16_mfma(dev(x), k1, b1, k10, b10, T, mfma=16)
    xs = _frames(x, T, sel).astype(np.float64)
    ref1 = pfnl_spec.lrelu(pfnl_spec.conv2d_same(xs, k1.astype(np.float64), b1.astype(np.float64)))
    bound1 = N.conv_bound(xs, k1, (b1,))
    assert np.abs(ref1).max() < N.F16_MAX / 4
    cat = _concat(ref1, T)
    refb = pfnl_spec.lrelu(pfnl_spec.conv2d_same(cat, k10.astype(np.float64), b10.astype(np.float64)))
    boundb = N.conv_bound(cat, k10, (b10,), xerr=_concat(bound1, T)) + 2.0 ** -22 * np.abs(refb) + 2.0 ** -36
    bound1 = bound1 + 2.0 ** -22 * np.abs(ref1) + 2.0 ** -36
    for name, got, ref, bound in (("inp1", _frames(o1.cpu().numpy(), T, sel), ref1, bound1), ("base", ob.cpu().numpy()[sel], refb, boundb)):
        got = np.asarray(got, np.float64)
        assert got.shape == ref.shape and np.isfinite(got).all(), name
        r = N.worst_ratio(got, ref, bound)
        print(f"bound ratio c1c10 mfma16 {name} ({geom}) {fam:8s} {r:.3f}")
        assert r <= 1.0, (name, geom, fam, r)


@pytest.mark.parametrize("nb,B,H,W", [(3, 4, 128, 128), (20, 4, 128, 128), (3, 2, 180, 318)])
def test_forward_c1c10_mfma16(nb, B, H, W):
    """The forward under the default option (split16_mfma=16: both launches of a block on the 16x16x32 shape where the plan says so) against
    FastOracle at ABS_TOL, five repeats bit for bit; split16_mfma=32 restores the 32x32x16 kernels for both launches.  configs[1] at 3 and 20
    blocks and a ragged shape (180 x 318: partial tiles on both edges) with at least one chain per CU."""
    geom = PFNLGeometry(num_block=nb)
    w = synth.synthetic_weights(geom, seed=nb)
    eng = PFNLEngine(geom, device=0)
    eng.load_weights(w)
    x = synth.uniform_clips(B, 7, H, W, seed=B + W)
    pl = eng.plan(B, H, W)
    assert eng.get_option("split16_mfma") == "16" and pl["c1_mfma"] == pl["mfma"], pl
    if _grid() == 256:
        assert pl["c1_mfma"] == 16, pl                                  # (MI355X: 256 / 460 chains, whole rounds)
    y = eng.forward(x)
    for rep in range(4):
        assert np.array_equal(y.view(np.uint32), eng.forward(x).view(np.uint32)), rep
    ref = pfnl_fast.FastOracle(w, 7, 4, nb).forward(x)
    err = float(np.abs(y - ref).max())
    eng.set_option("split16_mfma", "32")
    p32 = eng.plan(B, H, W)
    assert p32["mfma"] == 32 and p32["c1_mfma"] == 32, p32
    y32 = eng.forward(x)
    print(f"forward {nb} blocks {B}x7x{H}x{W} ({pl['structure']} c1_mfma={pl['c1_mfma']}): max |y - oracle| {err:.3g}, "
          f"32x32x16 {np.abs(y32 - ref).max():.3g}, |y16 - y32| {np.abs(y - y32).max():.3g}")
    assert err < ABS_TOL, err
    eng.close()
