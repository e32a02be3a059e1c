"""The bf16 model of tests/numerics.py, checked on the host: the rounding helpers against torch.bfloat16 on every pattern, tie and
neighbour of a tie; the fp32 restatement of the kernels' rounding points (bf16_emulate) inside bf16_interval on every family and in
every mode, with the share of outputs the interval pins to one value; the exact `ties` and identity expectations; and mutants of the
restatement that the interval (or, for round-half-away, the ties) must reject (test_gpu_bf16_numerics.py holds the kernels to the
same checks)."""
import numpy as np
import pytest

import numerics as N

torch = pytest.importorskip("torch")

CLIPS, T, H, W = 2, 3, 9, 38                    # two ragged 8 x 32 tile rows and columns
PINNED_FLOOR = 0.9                              # a condition on the inputs (normal, binades), from the reference alone


def _case(mode, fam, cout=64):
    rng = np.random.default_rng([N.BF16_MODES.index(mode), N.BF16_FAMILIES.index(fam)])
    return N.bf16_case(mode, fam, rng, CLIPS, T, H, W, cout=cout)


def _torch_bf16(v):
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def _finite_patterns():
    v = (np.arange(65536, dtype=np.uint32) << np.uint32(16)).view(np.float32)
    return v[np.isfinite(v)]


def test_bf16_round_is_torch_bfloat16():
    """bf16_round: idempotent on all bf16 patterns; on the fp32 midpoint of every pair of adjacent finite patterns it goes to the even
    one, on the fp32 neighbours either side of the midpoint to the nearer - all bit for bit what torch.bfloat16 does."""
    v = _finite_patterns()
    assert np.array_equal(N.bf16_round(v).view(np.uint32), v.view(np.uint32))
    allp = (np.arange(65536, dtype=np.uint32) << np.uint32(16)).view(np.float32)
    assert np.isnan(N.bf16_round(allp[np.isnan(allp)])).all()
    u = v.view(np.uint32)
    u = u[(u & np.uint32(0x7fff0000)) < np.uint32(0x7f7f0000)]                 # the pattern above it (in magnitude) is finite too
    mid = u | np.uint32(0x8000)
    for w in (mid, mid - np.uint32(1), mid + np.uint32(1)):
        f = w.view(np.float32)
        assert np.array_equal(N.bf16_round(f).view(np.uint32), _torch_bf16(f).view(np.uint32))
    want = np.where((u >> np.uint32(16)) & np.uint32(1), u + np.uint32(0x10000), u)   # the even neighbour
    assert np.array_equal(N.bf16_round(mid.view(np.float32)).view(np.uint32), want)
    assert np.array_equal(N.bf16_round((mid - np.uint32(1)).view(np.float32)).view(np.uint32), u)
    assert np.array_equal(N.bf16_round((mid + np.uint32(1)).view(np.float32)).view(np.uint32), u + np.uint32(0x10000))
    assert np.array_equal(N.bf16_round64(v.astype(np.float64)).view(np.uint32), v.view(np.uint32))   # fp64 helper: idempotent too
    assert np.array_equal(N.bf16_round64(mid.view(np.float32).astype(np.float64)).view(np.uint32), want)


def test_bf16_round64_rounds_once():
    """An fp64 value a hair off a bf16 tie goes to the neighbour on its side, not - through an fp32 tie - to the even one."""
    v = _finite_patterns()
    u = v.view(np.uint32)
    u = u[((u & np.uint32(0x7fff0000)) < np.uint32(0x7f7f0000)) & ((u & np.uint32(0x7fffffff)) != 0)]
    tie = (u | np.uint32(0x8000)).view(np.float32).astype(np.float64)
    up = N.bf16_round64(tie * (1 + 2.0 ** -40)).view(np.uint32)
    dn = N.bf16_round64(tie * (1 - 2.0 ** -40)).view(np.uint32)
    assert np.array_equal(up, u + np.uint32(0x10000))                           # away from zero: the upper neighbour in magnitude
    assert np.array_equal(dn, u)
    collapsed = N.bf16_round((tie * (1 + 2.0 ** -40)).astype(np.float32)).view(np.uint32)
    assert (collapsed != up).any()                                              # the two-step rounding is wrong on the even patterns


def _emulate(mode, kw, fault=None):
    if mode == "1x1":
        return N.bf16_emulate(N.concat_frames(kw["x"], T), kw["k"], kw["bias"], fault=fault)
    if mode == "merge":
        return N.bf16_emulate(N.concat_frames(kw["x"], T), kw["k"], kw["bias"], out_f32=True, fault=fault)
    return N.bf16_emulate(fault=fault, **kw)


def _spec(mode, kw, out1=None):
    """(r, e) of a mode; c1c10 with out1: of base, the 1x1 over that (rounded) out1."""
    if mode in ("1x1", "merge"):
        return N.bf16_spec(N.concat_frames(kw["x"], T), kw["k"], kw["bias"])
    if mode == "c1c10":
        if out1 is not None:
            return N.bf16_spec(N.concat_frames(out1, T), kw["k10"], kw["b10"])
        return N.bf16_spec(kw["x"], kw["k"], kw["bias"])
    return N.bf16_spec(**kw)


@pytest.mark.parametrize("mode", N.BF16_MODES)
def test_emulation_inside_the_interval(mode):
    """bf16_emulate inside bf16_interval (convmerge1, T = 3 and 48 channels: within e) on every family; the pinned share printed, and
    at least 0.9 on normal and binades."""
    for fam in N.BF16_FAMILIES:
        kw = _case(mode, fam, cout=48 if mode == "merge" else 64)
        got = _emulate(mode, kw)
        r, e = _spec(mode, kw)
        assert np.isfinite(r).all() and np.abs(r).max() + e.max() < 2.0 ** 127, (mode, fam)     # a condition on the inputs
        if mode == "merge":
            ratio = N.worst_ratio(got, r, e)
            print(f"bf16 emulation {mode:6s} {fam:10s} |got - r| / e worst {ratio:.3f}")
            assert ratio <= 1.0, (mode, fam, ratio)
            continue
        checks = [("", got, r, e)] if mode != "c1c10" else [("out1", got[0], r, e), ("base", got[1]) + _spec(mode, kw, out1=got[0])]
        for name, g, rr, ee in checks:
            out, pin, npin, match, c = N.bf16_report(g, rr, ee)
            print(f"bf16 emulation {mode:6s} {name:4s} {fam:10s} pinned {pin:.3f} ({match}/{npin} match)  outside {out:.4f}  smallest c {c:.3f}")
            assert out == 0.0 and match == npin, (mode, name, fam, out)
            if fam in ("normal", "binades"):
                assert pin >= PINNED_FLOOR, (mode, name, fam, pin)


def _ties_cases():
    rng = np.random.default_rng(7)
    x, bias, want = N.bf16_ties_plain(rng, (CLIPS * T, H, W, 64))
    plain = dict(x=x, k=N.identity_kernel(), bias=bias, act=False)
    a, resid, wantf = N.bf16_ties_fused(rng, CLIPS, T, H, W)
    xf = N.bf16_xdata(rng, "normal", (CLIPS * T, H, W, 64))
    fused = dict(x=xf, k=np.zeros((3, 3, 64, 64), np.float32), bias=np.zeros(64, np.float32), addend=a, add_div=T, resid=resid)
    return (plain, want), (fused, wantf)


def test_ties_and_identity_are_exact():
    """The exact constructions: every expectation is a bf16 tie resolved to even (both parities occur), the restatement gives it bit
    for bit, and the zero-bias identity returns its input (-0 as +0)."""
    (plain, want), (fused, wantf) = _ties_cases()
    for kw, w in ((plain, want), (fused, wantf)):
        assert np.array_equal(N.bf16_emulate(**kw).view(np.uint32), w.view(np.uint32))
        away = N.bf16_emulate(fault="half_away", **kw)
        assert 0.3 < (away != w).mean() < 0.7                       # about half the ties have an even lower neighbour
    x, wantx = N.identity_inputs(np.random.default_rng(8), (CLIPS * T, H, W, 64))
    got = N.bf16_emulate(x, N.identity_kernel(), np.zeros(64, np.float32), act=False)
    assert np.array_equal(got.view(np.uint32), wantx.view(np.uint32))
    assert np.signbit(x[x == 0]).any() and not np.signbit(got[x == 0]).any()


def test_mutants_fail():
    """Each wrong version of the restatement leaves the interval (round-half-away: misses the ties) where the right one passes."""
    share = {}

    def outside(mode, fam, fault):
        kw = _case(mode, fam)
        got = _emulate(mode, kw, fault=fault)
        if mode == "c1c10":                                         # base against the 1x1 over the mutant's own rounded out1
            return N.bf16_report(got[1], *_spec(mode, kw, out1=got[0]))[0]
        return N.bf16_report(got, *_spec(mode, kw))[0]

    for fam in ("normal", "binades"):
        share["trunc_store", fam] = outside("fused", fam, "trunc_store")
        share["round_before_resid", fam] = outside("fused", fam, "round_before_resid")
        share["half_away", fam] = outside("fused", fam, "half_away")
    share["trunc_weights", "normal"] = outside("plain", "normal", "trunc_weights")
    share["c10_unrounded", "normal"] = outside("c1c10", "normal", "c10_unrounded")
    share["addend_mod", "normal"] = outside("fused", "normal", "addend_mod")
    share["resid_first", "normal"] = outside("fused", "normal", "resid_first")
    for (fault, fam), s in share.items():
        print(f"bf16 mutant {fault:18s} {fam:8s} share outside the interval {s:.4f}")
        if fault != "half_away":
            assert s > 0.0, (fault, fam)
    assert share["trunc_store", "normal"] > 0.3 and share["trunc_store", "binades"] > 0.3
    assert share["round_before_resid", "normal"] > 0.05 and share["round_before_resid", "binades"] > 0.02
    # round-half-away differs from nearest-even on exact ties only: the interval does not see it, the ties do
    assert share["half_away", "normal"] < 1e-3
    for kw, want in _ties_cases():
        miss = float((N.bf16_emulate(fault="half_away", **kw) != want).mean())
        print(f"bf16 mutant half_away on ties: share wrong {miss:.3f}")
        assert miss > 0.3
