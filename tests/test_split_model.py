"""The host model of the split-f16 kernels' operands (tests/numerics.py), on the CPU: the split at binary16's edges, the error bound
against an fp64 emulation of the split, and the scales the split commutes with."""
import numpy as np
import pytest

import numerics as N

f32 = np.float32


def _parts(v):
    hi, lo = N.split_parts(np.array([v], np.float32))
    return float(hi[0]), float(lo[0])


def _bits(rng, n, nbits, e_lo=-12, e_hi=15):
    """Values with at most nbits significant bits, exponents in [e_lo, e_hi]."""
    m = rng.integers(2 ** (nbits - 1), 2 ** nbits, size=n).astype(np.float64)
    return (np.ldexp(m, rng.integers(e_lo, e_hi + 1, size=n) - nbits + 1) * rng.choice([-1.0, 1.0], size=n)).astype(np.float32)


def test_split_reconstructs_22_bit_values_exactly():
    rng = np.random.default_rng(0)
    for nbits in (1, 11, 12, 21, 22):
        x = _bits(rng, 20000, nbits)
        x = x[np.abs(x) < N.F16_MAX]
        assert np.array_equal(N.emulate(x), x.astype(np.float64)), nbits
    x = _bits(rng, 20000, 24)
    x = x[np.abs(x) < N.F16_MAX]
    assert not np.array_equal(N.emulate(x), x.astype(np.float64))         # 24 bits do not fit: the model is not the identity


def test_split_host_layout():
    """split_host: per pixel [channel half][hi 32 | lo' 32] binary16 bit patterns."""
    rng = np.random.default_rng(1)
    v = rng.normal(size=(3, 5, 64)).astype(np.float32)
    sf = N.split_host(v)
    hi, lo = N.split_parts(v)
    assert sf.shape == (3, 5, 128) and sf.dtype == np.int16
    for m in (0, 1):
        assert np.array_equal(sf[..., 64 * m:64 * m + 32], hi[..., 32 * m:32 * m + 32].view(np.int16))
        assert np.array_equal(sf[..., 64 * m + 32:64 * m + 64], lo[..., 32 * m:32 * m + 32].view(np.int16))


def test_split_signed_zeros():
    h, l = N.split_parts(np.array([0.0, -0.0], np.float32))
    assert h.view(np.uint16).tolist() == [0x0000, 0x8000]
    assert l.view(np.uint16).tolist() == [0x0000, 0x0000]                 # -0 - (-0) = +0
    assert N.emulate(np.array([-0.0], np.float32))[0] == 0.0


def test_split_binary16_ties_round_to_even():
    assert _parts(1.0 + 2.0 ** -11) == (1.0, 1.0)                          # tie: hi down to the even 1.0, lo' = 2^-11 * 2^11
    assert _parts(1.0 + 3 * 2.0 ** -11) == (1.0 + 2.0 ** -9, -1.0)        # tie: hi up to the even 1 + 2^-9, lo' < 0
    assert _parts(-(1.0 + 2.0 ** -11)) == (-1.0, -1.0)
    assert _parts(2048.0 + 1.0) == (2048.0, 2048.0)                        # 2049: ulp16 = 2, tie to even 2048; lo' = 1 * 2^11
    # the tie of lo' itself: (x - hi) 2^11 halfway between two binary16 numbers
    x = f32(1.0 + 2.0 ** -12 + 2.0 ** -23)                                 # x - hi = 2^-12 + 2^-23: 12 bits, lo' rounds it to 11
    h, l = _parts(x)
    assert h == 1.0 and l == 0.5                                          # 0.5 + 2^-12: a tie between 0.5 and 0.5 + 2^-11 -> even 0.5


def test_split_just_below_powers_of_two():
    for p in (-10, -1, 0, 3, 10):
        x = np.nextafter(f32(2.0 ** p), f32(0))
        h, l = _parts(x)
        assert h == 2.0 ** p                                              # hi rounds up a binade
        assert l < 0 and l == float(np.float16((float(x) - h) * 2048))
        assert N.emulate(np.array([x]))[0] == float(x)                    # x - hi = -ulp32: 1 bit


def test_split_subnormal_hi_and_zero_hi():
    for x in (2.0 ** -15 * 1.3, 2.0 ** -20 * 1.7, 2.0 ** -24, 2.0 ** -24 * 1.5, np.nextafter(f32(2.0 ** -14), f32(0))):
        x = f32(x)
        h, l = _parts(x)
        assert h == float(np.float16(x)) and abs(h) <= 2.0 ** -14         # hi is a binary16 subnormal (or 2^-14 itself by rounding)
        assert abs(float(x) - (h + l * 2.0 ** -11)) <= 2.0 ** -36         # the operand floor, not a relative bound
    for x in (2.0 ** -25 * 0.99, 2.0 ** -26, 2.0 ** -30):
        h, l = _parts(f32(x))
        assert h == 0.0 and l == float(np.float16(f32(x) * f32(2048)))    # hi = 0: lo' carries all of it
        assert abs(x - l * 2.0 ** -11) <= 2.0 ** -36
    h, l = _parts(f32(2.0 ** -36))
    assert h == 0.0 and l == 0.0                                          # 2^-25 after the scale: a tie to even 0


def test_split_top_of_the_domain():
    assert _parts(65504.0) == (65504.0, 0.0)
    h, l = _parts(65519.0)
    assert h == 65504.0 and l == 15.0 * 2048                               # just above 65504: hi = 65504, lo' holds the rest
    h, _ = _parts(65520.0)
    assert h == np.inf                                                    # the binary16 overflow (the forward's range flag)
    assert N.emulate(np.array([65000.123], np.float32))[0] == pytest.approx(65000.123, rel=2.0 ** -22)


def test_split_error_model():
    """|x - emulate(x)| <= max(2^-22 |x|, 2^-36) over binary16's range, and the floor only for |x| < 2^-12 (numerics docstring)."""
    rng = np.random.default_rng(2)
    x = np.ldexp(1.0 + rng.random(400000), rng.integers(-45, 15, size=400000)).astype(np.float32)   # |x| < 2^15
    e = np.abs(N.emulate(x) - x.astype(np.float64))
    assert (e <= np.maximum(2.0 ** -22 * np.abs(x), 2.0 ** -36)).all()
    assert (e[np.abs(x) >= N.FLOOR_BELOW] <= 2.0 ** -22 * np.abs(x[np.abs(x) >= N.FLOOR_BELOW])).all()
    assert e[np.abs(x) < 2.0 ** -16].max() > 2.0 ** -22 * 2.0 ** -16       # below 2^-14 the relative bound does not hold


def _emulated_conv(x, k):
    """conv2d_same with emulated split operands, exact products, an fp32 accumulator per product class (hi.hi; the cross products
    hi.lo' + lo'.hi x 2^11) summed sequentially, and the final accm + accc 2^-11 - the kernels' arithmetic on the host."""
    xh, xl = (p.astype(np.float64) for p in N.split_parts(x))
    kh, kl = (p.astype(np.float64) for p in N.split_parts(k))
    kh_, kw_, cin, cout = k.shape
    B, H, W, _ = x.shape
    pad = lambda a: np.pad(a, ((0, 0), (kh_ // 2, kh_ // 2), (kw_ // 2, kw_ // 2), (0, 0)))   # noqa: E731
    xh, xl = pad(xh), pad(xl)
    accm = np.zeros((B, H, W, cout), np.float32)
    accc = np.zeros((B, H, W, cout), np.float32)
    for dy in range(kh_):
        for dx in range(kw_):
            for c in range(cin):
                a_h, a_l = xh[:, dy:dy + H, dx:dx + W, c:c + 1], xl[:, dy:dy + H, dx:dx + W, c:c + 1]
                accm = (accm + a_h * kh[dy, dx, c]).astype(np.float32)
                accc = (accc + (a_h * kl[dy, dx, c] + a_l * kh[dy, dx, c])).astype(np.float32)
    return accm.astype(np.float64) + accc.astype(np.float64) * 2.0 ** -11


@pytest.mark.parametrize("scale_log2", [-30, -24, -20, -16, -14, -12, -6, 0, 8, 15])
def test_bound_holds_for_the_emulated_split(scale_log2):
    """The bound of numerics.conv_bound for the kernels' arithmetic emulated on the host (fp64 products, fp32 accumulators), at
    activation scales 2^-30 ... 2^15 (clamped to binary16's domain): what the GPU tests hold the kernels to is not beyond the design."""
    from oracle import pfnl_spec
    rng = np.random.default_rng(scale_log2 + 100)
    x = rng.normal(size=(2, 6, 7, 64)) * 2.0 ** scale_log2
    x = np.clip(x, -6.5e4, 6.5e4).astype(np.float32)
    k = (rng.normal(size=(3, 3, 64, 16)) / 24).astype(np.float32)
    got = _emulated_conv(x, k)
    ref = pfnl_spec.conv2d_same(x.astype(np.float64), k.astype(np.float64), None)
    r = N.worst_ratio(got, ref, N.conv_bound(x, k))
    assert r <= 1.0, r
    S, _ = N.conv_terms(x, k)
    if scale_log2 <= -20:                                                 # the floor is real there: alpha S alone does not hold
        assert N.worst_ratio(got, ref, N.alpha(576) * S) > 1.0


@pytest.mark.parametrize("fam", ["binades", "edges"])
def test_bound_holds_for_the_emulated_split_on_the_gpu_families(fam):
    from oracle import pfnl_spec
    rng = np.random.default_rng(len(fam))
    x = N.binades(rng, (1, 6, 7, 64)) if fam == "binades" else N.edges(rng, (1, 6, 7, 64))
    k = (rng.normal(size=(3, 3, 64, 16)) / 24).astype(np.float32) if fam == "binades" else N.edge_weights(rng, (3, 3, 64, 16))
    got = _emulated_conv(x, k)
    ref = pfnl_spec.conv2d_same(x.astype(np.float64), k.astype(np.float64), None)
    assert N.worst_ratio(got, ref, N.conv_bound(x, k)) <= 1.0


def test_the_bound_sees_a_flushed_subnormal():
    """What the GPU tests are for: the same emulation with binary16 subnormal operands flushed (what an MFMA that flushes would do)
    breaks the bound on dark data by orders of magnitude."""
    from oracle import pfnl_spec
    rng = np.random.default_rng(9)
    x = (rng.normal(size=(1, 5, 6, 64)) * 2.0 ** -16).astype(np.float32)
    k = (rng.normal(size=(3, 3, 64, 16)) / 24).astype(np.float32)
    hi, lo = N.split_parts(x)
    sub = lambda a: np.where(np.abs(a.astype(np.float64)) < 2.0 ** -14, 0.0, a.astype(np.float64))   # noqa: E731
    flushed = (sub(hi) + sub(lo) * 2.0 ** -11).astype(np.float32)       # (rounding the sum to fp32 adds at most 2^-24 relative)
    ref = pfnl_spec.conv2d_same(x.astype(np.float64), k.astype(np.float64), None)
    got = pfnl_spec.conv2d_same(flushed.astype(np.float64), k.astype(np.float64), None)
    assert N.worst_ratio(got, ref, N.conv_bound(x, k)) > 100.0


def test_equivariant_scales():
    rng = np.random.default_rng(4)
    assert N.equivariant_scales(rng.normal(size=100000).astype(np.float32), range(-20, 21)) == [0]
    unit = N.unit_binades(rng, (100000,))
    assert np.abs(unit).min() >= 0.25 and np.abs(unit).max() < 4.0
    assert N.equivariant_scales(unit, range(-20, 21)) == list(range(-10, 14))
