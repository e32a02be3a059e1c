"""The bf16 trunk kernels held to ONE bf16 rounding of the fp64 result (tests/numerics.py has the model; precision=bf16, BASELINE.json
configs[3]).

Every operand of these kernels is a bf16 number, every product exact in fp32, accumulation and epilogue fp32, one nearest-even rounding
at the store.  So for every hook and data family, element-wise:

    bf16(r - e) <= got <= bf16(r + e),   r: the fp64 spec on the bf16 inputs and bf16_round-ed weights,  e = (alpha(K) + n_e 2^-24) S

Where [r - e, r + e] holds no rounding boundary the output is pinned to one bf16 value (over 90 % of the outputs on N(0, 1) data and
on binades: tests/test_bf16_numerics_host.py checks that share on the same families): a store that truncates, an epilogue that rounds
twice, a pack that rounds the weights wrongly or a wrong addend index leave the interval on 8 - 55 % of the outputs.  The exact `ties`
constructions tell round-half-even from round-half-away, which no interval can.  Every call is made twice and must repeat bit for
bit.  Per test the pinned share, the pinned elements that matched and the smallest factor c for which bf16_interval(r, c e) would admit
every element are printed (-s); the assertion is at c = 1.

Geometries (T, clips, H, W): (3, 2, 9, 38) two ragged 8 x 32 tile rows and columns, (7, 1, 8, 32) exactly one tile, (5, 1, 1, 1),
(3, 1, 2, 2); grid + 1 clips of 8 x 32 (more chains than workgroups); the split geometries T7-s2-uneven and nfull0-ragged of
test_gpu_bf16.py.  The tests named *_default go through the hooks whose kernel PFNL_BF16_V3 / PFNL_CONV0 choose;
test_bf16_other_kernel_assignments runs them again under each other assignment in a process of its own."""
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import numerics as N  # noqa: E402
from oracle import pfnl_spec  # noqa: E402
from pfnl_amd import ops  # noqa: E402

FAMILIES = N.BF16_FAMILIES
GEOMS = [(3, 2, 9, 38), (7, 1, 8, 32), (5, 1, 1, 1), (3, 1, 2, 2)]
SPLITS = {"T7-s2-uneven": (7, 3, 13, 40, (0, 2, 4)), "nfull0-ragged": (7, 2, 11, 45, (0, 3, 3))}    # test_gpu_bf16.py _split_case
CONV0_FAMILIES = ["normal", "binades", "edges", "dark16", "dark20"]
CONV0_GEOMS = [(1, 7, 16, 24), (2, 3, 10, 38), (1, 5, 2, 2)]                                         # (B, T, H, W)


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _grid():
    """The grid of the persistent launches on this device (persistent_grid: the CU count rounded down to whole XCDs, at least 8)."""
    return max(8, torch.cuda.get_device_properties(0).multi_processor_count // 8 * 8)


def dev16(a):
    """bf16 values held as fp32 -> a bfloat16 device tensor (exact)."""
    assert not (np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) & np.uint32(0xffff)).any()
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).cuda()


def host(t):
    return t.float().cpu().numpy()


def _twice(run):
    """The hook's outputs as fp32 numpy arrays (a tuple for two outputs); a second call must give the same bits."""
    a, b = run(), run()
    one = not isinstance(a, tuple)
    a, b = ((a,), (b,)) if one else (a, b)
    for u, v in zip(a, b):
        assert torch.equal(u.view(torch.int16) if u.dtype == torch.bfloat16 else u.view(torch.int32),
                           v.view(torch.int16) if v.dtype == torch.bfloat16 else v.view(torch.int32)), "the call does not repeat bit for bit"
    out = tuple(host(u) for u in a)
    return out[0] if one else out


def _check(kernel, fam, got, r, e):
    """lo <= got <= hi element-wise at c = 1; prints the pinned share, the pinned elements that matched and the smallest c."""
    assert got.shape == r.shape, (got.shape, r.shape)
    assert np.isfinite(r).all() and np.abs(r).max() + e.max() < 2.0 ** 127, (kernel, fam, "the inputs leave bf16's range")
    assert np.isfinite(got).all(), (kernel, fam)
    outside, pin, npin, match, c = N.bf16_report(got, r, e)
    print(f"bf16 interval {kernel:40s} {fam:10s} pinned {pin:.3f} ({match}/{npin} match)  outside {outside:.5f}  smallest c {c:.3f}")
    assert outside == 0.0, (kernel, fam, outside, c)


def _sel(a, T, clips):
    """The frames of the clips `clips` of a per-frame array."""
    return np.concatenate([a[c * T:(c + 1) * T] for c in clips])


# ---- the launches, each as (inputs of numerics.bf16_case) -> outputs -----------------------------------------------------------

def _run_plain(kw, act, mfma=None, T=1):
    x, k, b = dev16(kw["x"]), kw["k"], kw["bias"]
    if mfma is None:
        return _twice(lambda: ops.conv3x3_bf16(x, k, b, act=act))
    za = torch.zeros((x.shape[0] // T,) + tuple(x.shape[1:]), dtype=torch.bfloat16, device="cuda")   # the third-generation kernel's plain
    zr = torch.zeros_like(x)                                               # form: the fused mode with zero addend and residual
    return _twice(lambda: ops.conv3x3_bf16_ex(x, k, b, za, T, zr, act=act, mfma=mfma))


def _run_fused(kw, mfma=None, split=(0, 0, 0)):
    x, a, res = dev16(kw["x"]), dev16(kw["addend"]), dev16(kw["resid"])
    if mfma is None:
        return _twice(lambda: ops.conv3x3_bf16(x, kw["k"], kw["bias"], act=True, addend=a, add_div=kw["add_div"], resid=res))
    return _twice(lambda: ops.conv3x3_bf16_ex(x, kw["k"], kw["bias"], a, kw["add_div"], res, mfma=mfma, split=split))


def _run_c1c10(kw, mfma=None, split=(0, 0, 0)):
    x = dev16(kw["x"])
    if mfma is None:
        return _twice(lambda: ops.conv1_conv10_bf16(x, kw["k"], kw["bias"], kw["k10"], kw["b10"], kw["T"]))
    return _twice(lambda: ops.conv1_conv10_bf16_ex(x, kw["k"], kw["bias"], kw["k10"], kw["b10"], kw["T"], mfma=mfma, split=split))


def _check_fused(name, fam, kw, got, clips=None):
    T = kw["add_div"]
    if clips is not None:
        kw = dict(kw, x=_sel(kw["x"], T, clips), addend=kw["addend"][clips], resid=_sel(kw["resid"], T, clips))
        got = _sel(got, T, clips)
    _check(name, fam, got, *N.bf16_spec(**kw))


def _check_c1c10(name, fam, kw, out1, base, split_s=0, clips=None):
    """out1 against the spec; base against the spec of the 1x1 over the kernel's own - already checked - out1 (a cut chain's base is
    finished from split_s raw fp32 partial sums: n_e = 2 + split_s)."""
    T = kw["T"]
    x = kw["x"]
    if clips is not None:
        x, out1, base = _sel(x, T, clips), _sel(out1, T, clips), base[clips]
    _check(name + " out1", fam, out1, *N.bf16_spec(x, kw["k"], kw["bias"]))
    _check(name + " base", fam, base, *N.bf16_spec(N.concat_frames(out1, T), kw["k10"], kw["b10"], n_e=2 + split_s))


# ---- the default hooks (the kernels PFNL_BF16_V3 assigns) -----------------------------------------------------------------------

@pytest.mark.parametrize("act", [True, False])
@pytest.mark.parametrize("fam", FAMILIES)
def test_bf16_plain_default(fam, act):
    """ops.conv3x3_bf16 without addend: out = act(conv + bias), n_e = 2."""
    for T, clips, H, W in GEOMS:
        kw = N.bf16_case("plain", fam, _rng("plain", fam, act, T, H, W), clips, T, H, W)
        _check(f"plain act={int(act)} {clips * T}x{H}x{W}", fam, _run_plain(kw, act), *N.bf16_spec(act=act, **kw))


@pytest.mark.parametrize("fam", FAMILIES)
def test_bf16_fused_default(fam):
    """ops.conv3x3_bf16 with addend and resid: out = act(conv + bias + addend[item / T]) + resid, n_e = 4."""
    for T, clips, H, W in GEOMS:
        kw = N.bf16_case("fused", fam, _rng("fused", fam, T, H, W), clips, T, H, W)
        _check_fused(f"fused {clips}x{T}x{H}x{W}", fam, kw, _run_fused(kw))


@pytest.mark.parametrize("fam", FAMILIES)
def test_bf16_c1c10_default(fam):
    """ops.conv1_conv10_bf16: conv1_i + conv10_i in one launch."""
    for T, clips, H, W in GEOMS:
        kw = N.bf16_case("c1c10", fam, _rng("c1c10", fam, T, H, W), clips, T, H, W)
        _check_c1c10(f"c1c10 {clips}x{T}x{H}x{W}", fam, kw, *_run_c1c10(kw))


def _ties(mfma):
    """The exact constructions on one MFMA form (None: the default hooks): plain ties, the zero-bias identity, fused ties."""
    T, clips, H, W = 3, 2, 9, 38
    rng = _rng("ties")
    x, bias, want = N.bf16_ties_plain(rng, (clips * T, H, W, 64))
    got = _run_plain(dict(x=x, k=N.identity_kernel(), bias=bias), False, mfma, T)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), (mfma, "plain ties", int(bad.sum()), x[bad][:4], got[bad][:4], want[bad][:4])
    xi, wanti = N.identity_inputs(rng, (clips * T, H, W, 64))
    got = _run_plain(dict(x=xi, k=N.identity_kernel(), bias=np.zeros(64, np.float32)), False, mfma, T)
    bad = got.view(np.uint32) != wanti.view(np.uint32)
    assert not bad.any(), (mfma, "identity", int(bad.sum()), xi[bad][:4], got[bad][:4])
    a, resid, wantf = N.bf16_ties_fused(rng, clips, T, H, W)
    kw = dict(x=N.bf16_xdata(rng, "normal", (clips * T, H, W, 64)), k=np.zeros((3, 3, 64, 64), np.float32), bias=np.zeros(64, np.float32),
              addend=a, add_div=T, resid=resid)
    got = _run_fused(kw, mfma)
    bad = got.view(np.uint32) != wantf.view(np.uint32)
    assert not bad.any(), (mfma, "fused ties", int(bad.sum()), got[bad][:4], wantf[bad][:4])


def test_bf16_ties_and_identity_default():
    """Exact answers, bit for bit: x + bias and addend + resid that lie exactly between two bf16 numbers go to the even one; the
    zero-bias identity returns its input (numerics.bf16_ties_plain, bf16_ties_fused, identity_inputs)."""
    _ties(None)


@pytest.mark.parametrize("fam", CONV0_FAMILIES)
def test_bf16_conv0_default(fam):
    """ops.conv0_bf16 (launch_conv0_bf16, which feeds the whole bf16 trunk): bit-equal to bf16_round of ops.conv0 in the same process -
    the same template, only the store differs - and inside the interval of the fp64 spec with the slack of the split-f16 conv0
    (alpha(75) S + beta A, test_gpu_strict_numerics.py; the VALU kernel of PFNL_CONV0=valu needs alpha(75) S only)."""
    for B, T, H, W in CONV0_GEOMS:
        rng = _rng("conv0", fam, T, H, W)
        shape = (B, T, H, W, 3)
        x = {"normal": lambda: rng.normal(size=shape).astype(np.float32), "binades": lambda: N.binades(rng, shape),
             "edges": lambda: N.edges(rng, shape)}.get(fam, lambda: N.dark(rng, shape, 2.0 ** -int(fam[4:])))()
        k = N.edge_weights(rng, (5, 5, 3, 64)) if fam == "edges" else (rng.normal(size=(5, 5, 3, 64)) / np.sqrt(75)).astype(np.float32)
        b = N.bf16_bias(rng, fam, 64)
        xd = torch.from_numpy(x).cuda()
        got = _twice(lambda: ops.conv0_bf16(xd, k, b))
        f32 = ops.conv0(xd, k, b).cpu().numpy()
        assert np.array_equal(got.view(np.uint32), N.bf16_round(f32).view(np.uint32)), (fam, B, T, H, W)
        xf = x.reshape(B * T, H, W, 3)
        r = pfnl_spec.lrelu(pfnl_spec.conv2d_same(xf.astype(np.float64), k.astype(np.float64), b.astype(np.float64)))
        _check(f"conv0 {B}x{T}x{H}x{W}", fam, got, r, N.conv_bound(xf, k, (b,)))


# ---- the third-generation kernel's two MFMA forms, uncut and split (the _ex hooks; PFNL_BF16_V3 changes nothing here) -----------------

@pytest.mark.parametrize("mfma", [32, 16])
@pytest.mark.parametrize("fam", FAMILIES)
def test_bf16_fused_ex(fam, mfma):
    for T, clips, H, W in GEOMS:
        kw = N.bf16_case("fused", fam, _rng("fused", fam, T, H, W), clips, T, H, W)
        _check_fused(f"fused mfma{mfma} {clips}x{T}x{H}x{W}", fam, kw, _run_fused(kw, mfma))
    for name, (T, clips, H, W, split) in SPLITS.items():
        kw = N.bf16_case("fused", fam, _rng("fused", fam, name), clips, T, H, W)
        _check_fused(f"fused mfma{mfma} split {name}", fam, kw, _run_fused(kw, mfma, split))


@pytest.mark.parametrize("mfma", [32, 16])
@pytest.mark.parametrize("fam", FAMILIES)
def test_bf16_c1c10_ex(fam, mfma):
    for T, clips, H, W in GEOMS:
        kw = N.bf16_case("c1c10", fam, _rng("c1c10", fam, T, H, W), clips, T, H, W)
        _check_c1c10(f"c1c10 mfma{mfma} {clips}x{T}x{H}x{W}", fam, kw, *_run_c1c10(kw, mfma))
    for name, (T, clips, H, W, split) in SPLITS.items():
        kw = N.bf16_case("c1c10", fam, _rng("c1c10", fam, name), clips, T, H, W)
        _check_c1c10(f"c1c10 mfma{mfma} split {name}", fam, kw, *_run_c1c10(kw, mfma, split), split_s=split[1])


@pytest.mark.parametrize("mfma", [32, 16])
def test_bf16_ties_and_identity_ex(mfma):
    """The exact constructions on both MFMA forms of the third-generation kernel (its plain form: act off, zero addend and residual)."""
    _ties(mfma)


@pytest.mark.parametrize("mfma", [32, 16])
@pytest.mark.parametrize("fam", ["normal", "bf16_edges"])
@pytest.mark.parametrize("mode", ["fused", "c1c10"])
def test_bf16_more_chains_than_workgroups(mode, fam, mfma):
    """grid + 1 clips of 8 x 32 pixels (one chain each), T = 3: the spec on the first clip, the last clip of the first round and the
    one clip of the second round; every clip repeats bit for bit."""
    G = _grid()
    T, clips, H, W = 3, G + 1, 8, 32
    sel = [0, G - 1, G]
    kw = N.bf16_case(mode, fam, _rng("chains", mode, fam), clips, T, H, W)
    if mode == "fused":
        _check_fused(f"fused mfma{mfma} {clips} chains", fam, kw, _run_fused(kw, mfma), clips=sel)
    else:
        _check_c1c10(f"c1c10 mfma{mfma} {clips} chains", fam, kw, *_run_c1c10(kw, mfma), clips=sel)


# ---- the 1x1 and convmerge1 (one kernel each, whatever the environment) ---------------------------------------------------------------

@pytest.mark.parametrize("T", [3, 5, 7])
@pytest.mark.parametrize("fam", FAMILIES)
def test_bf16_conv1x1(fam, T):
    """ops.conv1x1_bf16 (conv10_i as its own launch): K = 64 T, n_e = 2; 342 pixels (no multiple of a wave's 32), and one."""
    for items, H, W in ((2, 9, 38), (1, 1, 1)):
        kw = N.bf16_case("1x1", fam, _rng("1x1", fam, T, H), items, T, H, W)
        x = dev16(kw["x"])
        got = _twice(lambda: ops.conv1x1_bf16(x, kw["k"], kw["bias"], act=True, frames_per_item=T))
        _check(f"1x1 T={T} {items}x{H}x{W}", fam, got, *N.bf16_spec(N.concat_frames(kw["x"], T), kw["k"], kw["bias"]))


@pytest.mark.parametrize("cout", [48, 64])
@pytest.mark.parametrize("T", [3, 7])
@pytest.mark.parametrize("fam", FAMILIES)
def test_bf16_convmerge1(fam, T, cout):
    """ops.conv3x3_accum_bf16: fp32 out, no store rounding: |got - r| <= e with K = 576 T, n_e = 2; channels >= cout exactly 0."""
    for clips, H, W in ((2, 9, 38), (1, 8, 32), (1, 2, 2)):
        kw = N.bf16_case("merge", fam, _rng("merge", fam, T, cout, H), clips, T, H, W, cout=cout)
        x = dev16(kw["x"])
        got = _twice(lambda: ops.conv3x3_accum_bf16(x, kw["k"], kw["bias"], act=True, frames_per_clip=T))
        r, e = N.bf16_spec(N.concat_frames(kw["x"], T), kw["k"], kw["bias"])
        assert np.isfinite(got).all() and np.abs(r).max() + e.max() < 2.0 ** 127
        ratio = N.worst_ratio(got[..., :cout], r, e)
        print(f"bf16 bound    {'convmerge1 T=%d cout=%d %dx%dx%d' % (T, cout, clips, H, W):40s} {fam:10s} |got - r| / e worst {ratio:.3f}")
        assert ratio <= 1.0, (fam, T, cout, ratio)
        assert not got[..., cout:].any()


# ---- the other kernel assignments, each in a process of its own -----------------------------------------------------------------------

@pytest.mark.parametrize("sel", ["v2+valu", "v3-all", "v3-mode2"])
def test_bf16_other_kernel_assignments(sel):
    """By default the hooks above reach the second-generation 3x3 kernel for the plain mode only, the third-generation one for the
    chained modes only, and never conv0's VALU kernel.  PFNL_BF16_V3 = 0 / 1 / 2 and PFNL_CONV0 = valu assign the kernels otherwise;
    both are read once per process, so each setting runs this file's *_default tests in a fresh child (which stops at its first failure)."""
    extra = {"v2+valu": {"PFNL_BF16_V3": "0", "PFNL_CONV0": "valu"}, "v3-all": {"PFNL_BF16_V3": "1"}, "v3-mode2": {"PFNL_BF16_V3": "2"}}[sel]
    env = dict(os.environ, **extra)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-s", "-m", "gpu", "-k", "default"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print("\n".join(f"[{sel}] {line.lstrip('.')}" for line in r.stdout.splitlines() if line.lstrip(".").startswith("bf16 ")))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-500:]
    assert " passed" in r.stdout and "failed" not in r.stdout
