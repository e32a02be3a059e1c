"""Host model of the exact fp32 split the f16-pipe kernels run on, and the error bound the split-f16 op tests hold them to.

THE SPLIT (conv_split16.h): an fp32 value x becomes two binary16 operands, hi = f16(x) and lo' = f16((x - hi) 2^11), both rounded to
nearest even; x - hi and the scaling are exact in fp32.  The kernels multiply hi.hi on one accumulator and the cross products
hi.lo' + lo'.hi on a second one that is scaled by 2^-11 at the end (the lo'.lo' product is dropped).  The operand they work on is
therefore emulate(x) = hi + lo' 2^-11:

  - |x - hi| <= 2^-11 |x| and lo' keeps 11 bits of it: |x - emulate(x)| <= 2^-22 |x| while lo' is a normal binary16 number;
  - lo' is a binary16 subnormal when |x - hi| < 2^-25, its step is then 2^-24: |x - emulate(x)| <= 2^-25 2^-11 = 2^-36 absolute.
    Below 2^-14 hi itself is subnormal and below 2^-25 it is 0, but x - hi then lies under 2^-25 and only lo' carries the value:
    the same 2^-36 floor.  So a split operand keeps all its 22 bits only above roughly 2^-14 (where lo' leaves the subnormal range
    for most values); at 2^-24 it keeps about 12 bits, at 2^-36 none.  This is the lower edge of the kernels' "fp32-FMA-chain
    accuracy": by design, not by a flush.
  - above 65504 hi rounds to 65504 up to 65520 and to infinity from there (the range flag of the forward, include/pfnl_hip.h).

THE BOUND, element-wise against the fp64 spec, for an output that sums K products a_i b_i (plus bias / addend / resid c_j):

    |got - ref| <= alpha(K) S + beta A,   S = sum |a_i b_i| + sum |c_j|,   A = sum (|a_i| [|b_i| < 2^-12] + |b_i| [|a_i| < 2^-12])

  - the operand error is |x - emulate(x)| <= max(2^-22 |x|, 2^-36), and the floor 2^-36 is reached only for |x| < 2^-12: above it
    x - hi is a multiple of ulp32(x) >= 2^-35, so lo' is a multiple of 2^-24 and exact even when it is subnormal.  A therefore
    counts an operand |a_i| only when its partner b_i is under 2^-12 (and vice versa): sum (|a_i| + |b_i|) restricted to the
    products a floor can touch.  Without the restriction one large activation would hide the floor of every small one.
  - beta = 2^-35: a product of two split operands is off by at most |e_a| |b| + |a| |e_b| + |e_a e_b|; the floor part of the e's is
    2^-36 each, so beta A is twice what the floor can contribute.  An MFMA that flushed binary16 subnormal inputs would lose a whole
    hi (up to 2^-14) or lo' (up to 2^-25 after the 2^-11 scale): 2^10 ... 2^21 times beta.
  - alpha(K): the accumulation is an fp32 FMA chain (fp32 A/B MFMA) or an fp32 accumulator fed exact f16 x f16 products (f16 MFMA).
    An fp32 FMA chain (v_mfma_f32_32x32x2_f32 is one, bit for bit) measures 0.75 - 1.5e-7 S for K <= 1024 on data of one scale,
    where the partial sums stay ~sqrt(K) below S.  On data spread over many binades a few terms carry S and every later rounding
    is a step of up to 2^-24 |partial| ~ 2^-24 S: K such steps, uniform and independent, have the standard deviation
    2^-24 sqrt(K / 3) S (8.3e-7 S at K = 576); the chain term is sqrt(3) of that, 2^-24 sqrt(K) S, as the worst of thousands of
    outputs sits near 2 standard deviations.  The split adds, per product, the normal-range part of the operand errors plus the
    dropped lo'.lo': 2^-22 S with independent signs.  So alpha(K) = 2^-24 sqrt(K) + 2^-22.  A sequential fp32 chain emulated on
    the edge data reaches 0.45 - 0.6 of it at K = 448 - 576 and ~0.2 at K = 4032; on the MI355X the f32-MFMA kernels reach up to
    0.65 and the split-f16 kernels up to 0.53 (test_gpu_numerics.py prints the ratios).  The f32-MFMA kernels must meet
    alpha(K) S on the same data (they have no beta term).

THE WINOGRAD MODEL (conv_wino.hip, conv_wino_ws.hip: F(2x2,3x3), the strict-fp32 3x3 kernels).  A 2x2 output tile at an even origin
comes from the 4x4 input tile d around it (zero padding, even H and W) and the filter g:

    Y = A^T [ U .* (B^T d B) ] A  summed over the input channels,   U = fp32(G g G^T)  (fp64 on the host, rounded once)

    B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]    G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1]    A^T = [1 1 1 0; 0 1 -1 -1]

An output's error does not scale with its own nine taps: every rounding acts on a quantity made of the whole 4x4 tile and the
transformed filter, and the cancellation that turns those into the nine-tap sum happens afterwards.  The magnitude that bounds every
intermediate of output (p, q) is therefore

    S_w = |A^T| [ |U| .* (|B^T| |d| |B|) ] |A|   summed over the input channels  (+ |bias|, |addend|, |resid| as in S)

and the bound is |got - ref| <= alpha_wino(K) S_w, alpha_wino(K) = 2^-24 (sqrt(K) + 7 + e), one 2^-24 S_w per rounding that every
output passes through, the roundings of the fixed stages added linearly (worst case), the chain's statistically as in alpha:

  - input transform, 2: t = d_a +- d_b (one fma with +-1: |error| <= 2^-24 (|d_a| + |d_b|)), then v = t_a +- t_b; both stages
    together are off by at most 2 2^-24 (|B^T| |d| |B|), which the rest of the formula carries to 2 2^-24 S_w;
  - U's one rounding, 1: 2^-24 |U| per element;
  - the chain over the K input channels of one accumulator (fp32 FMAs, each product exact): every step rounds a partial sum that
    is at most sum |U| |V| of its position, at most S_w after |A^T| . |A|: 2^-24 sqrt(K) S_w, the convention of alpha;
  - output transform, 4: two stages (over nu, then over xi) of two additions each, every partial result at most S_w;
  - the epilogue, e: one per addition (bias; the addend or mode 2's LDS partial; the residual) and one for the activation's
    multiplication by fp32(0.2) (which is off 0.2 by 2^-26 relative and scales everything before it by 0.2: under one 2^-24 S_w).
    Mode 0 (act(conv + bias)) and mode 3 (convmerge1): e = 2, alpha_wino = 2^-24 (sqrt(K) + 9).  Mode 1 (+ addend, + resid) and
    mode 2 (conv2_i: + the base half's partial from LDS, + bias, act, + resid): e = 4.
  - K: 64 in modes 0 and 1.  Mode 2 runs two chains of 64 (the base half's finished partial goes through its own output transform,
    is rounded into LDS as an fp32 value and added in the frame half's epilogue): sqrt(64) on each half's share of S_w, and
    the base half's own 2 + 1 + 4 roundings act on its share only, so 2^-24 (sqrt(128) + 7 + 4) (S_w over all 128 channels)
    covers it.  Mode 3 keeps one accumulator over all T frames: K = 64 T.
The kernels differ from the textbook form in two places that change no magnitude: Winograd row 2 is computed as d1 - d2 with -U, and
the persistent kernel's second output of each stage is m1 - (m2 + m3) where the per-tile kernel's is (m1 - m2) - m3.
wino_emulate_f32 restates the algorithm in numpy fp32 with the kernels' order of operations; on the families below it stays under
0.35 alpha_wino S_w (tests/test_wino_numerics_host.py prints the ratios; on the MI355X the kernels reach up to 0.46 with the rms of
err / S_w equal to the emulation's: test_gpu_strict_numerics.py), while against alpha(576) S it is off by a factor of
thousands on the edge data - the direct kernels' bound cannot be reused.

THE BF16 MODEL (conv_bf16.hip, conv_bf16_v2.hip, conv_bf16_v3.hip, conv0_kernel<true> / conv0_mfma_kernel<true>: precision=bf16).  Every
operand of these kernels is a bf16 number - the activations as they arrive, the weights rounded once by bf16_rne on the host - so every
product has 16 significant bits and is exact in fp32.  Accumulation and epilogue are fp32, and the result is rounded ONCE, to nearest
even, at the store.  The stored value is therefore the nearest-even bf16 of a number v within e of the fp64 result r, and since that
rounding is monotone

    bf16(r - e) <= got <= bf16(r + e)   element-wise,   e = (alpha(K) + n_e 2^-24) S          (bf16_interval, bf16_slack)

  - r: the fp64 spec on the bf16 inputs and the bf16_round-ed weights; S = sum |a_i b_i| + |bias| + |addend| + |resid| on the same
    operands (conv_terms).  Where the interval [r - e, r + e] holds no rounding boundary, lo == hi: the output is PINNED to one bf16
    value and the test is bit-exact there (96 % of the outputs on N(0, 1) data and on binades at K = 576); elsewhere two neighbours
    are admitted - cancellation the fp32 sum cannot resolve, not a tolerance.  S = 0 gives e = 0: the answer is exact.
  - alpha(K) is the constant above, unchanged: the chain's 2^-24 sqrt(K) plus 2^-22.  The bf16 operands need no 2^-22 (there is no
    split to be inexact); it stays because alpha is the figure the f32- and f16-MFMA kernels were measured against (at most 0.65),
    and the MFMA's summation inside a K = 16 / 32 block is not specified beyond "fp32".
  - n_e: one 2^-24 S per fp32 epilogue operation every output passes through, added linearly as in the Winograd model: the bias
    addition and the activation's multiplication by fp32(0.2) (plain launch, conv10_i / the 1x1, convmerge1: n_e = 2); the fused
    launch adds the addend and the residual (4); conv10_i of a cut chain is finished by c10_finalize_bf16_kernel, which adds split_s
    raw fp32 partial sums before the bias (2 + split_s).  The leaky-relu is a contraction (|lrelu(u) - lrelu(v)| <= |u - v|), so
    the error in front of it passes through it unamplified.
  - conv10_i inside the conv1_i + conv10_i launch reads conv1_i's ROUNDED tile from LDS: its spec is the 1x1 over the kernel's own
    out1 (checked first), not over the fp64 out1.
  - the fp32-output kernel (convmerge1, conv3x3_accum_bf16) has no store rounding: |got - r| <= e with K = 576 T.
  - exact cases (bf16_ties): with a one-hot centre tap of weight 1 and a bias of +-2^(E - 8) on inputs of binade E the fp32 value in
    front of the store is exact and lies exactly between two bf16 numbers (or, where the signs differ at the bottom of the binade,
    on one); likewise zero weights, addend a > 0 of binade E and resid 2^(E - 8) in the fused launch.  The expectation is then
    bf16_round(r) bit for bit: this is what tells round-half-even from round-half-away, which no interval can.  With a zero bias
    the identity returns its input bit for bit - except that -0 comes back as +0, the accumulator starting from the bias +0
    ((+0) + (-0) = +0 in IEEE arithmetic, and the other 575 products are zeros of either sign).
bf16_emulate restates the rounding points in numpy fp32 (a sequential chain, exact products, + bias, + addend, max(o, 0.2f o), + resid,
one RNE store; conv10_i from the rounded out1) and carries the faults of tests/test_bf16_numerics_host.py: a truncating store puts 48 %
of the outputs outside the interval, a second rounding in front of "+ resid" 25 % on N(0, 1) data and 8 % on binades.  On the MI355X the
kernels need at most 0.10 of e (3x3, 1x1), 0.26 (convmerge1) and 0.28 (conv0, against the split-f16 slack): test_gpu_bf16_numerics.py prints it.
"""
import numpy as np

SPLIT_SHIFT = 11                    # lo' = f16((x - hi) 2^11)
F16_MAX = 65504.0
BETA = 2.0 ** -35
FLOOR_BELOW = 2.0 ** -12            # operands that can reach the 2^-36 floor


def split_parts(x):
    """(hi, lo') of every element of an fp32 array, as binary16 arrays: hi = f16(x), lo' = f16((x - hi) 2^11), nearest even."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        hi = x.astype(np.float16)
        lo = ((x - hi.astype(np.float32)) * np.float32(2.0 ** SPLIT_SHIFT)).astype(np.float16)
    return hi, lo


def split_host(v):
    """The split format of an fp32 array [..., 64] as the kernels build it (conv_split16.h): per pixel [channel half][hi 32 | lo' 32]
    binary16, hi = f16(x) (nearest even), lo' = f16((x - hi) 2^11) - x - hi and the scaling are exact in fp32, one rounding each."""
    hi, lo = split_parts(v)
    hi, lo = hi.reshape(v.shape[:-1] + (2, 32)), lo.reshape(v.shape[:-1] + (2, 32))
    return np.concatenate([hi, lo], axis=-1).reshape(v.shape[:-1] + (128,)).view(np.int16)


def emulate(x):
    """The operand the kernels multiply: hi + lo' 2^-11, in fp64."""
    hi, lo = split_parts(x)
    return hi.astype(np.float64) + lo.astype(np.float64) * 2.0 ** -SPLIT_SHIFT


def alpha(K):
    """Error per unit of S of a K-product sum: the fp32 chain's 2^-24 sqrt(K) plus the split's 2^-22 (module docstring)."""
    return 2.0 ** -24 * np.sqrt(K) + 2.0 ** -22


def conv_terms(x, k, extra=()):
    """S and A of the bound for conv2d_same(x, k) (fp64, [B, H, W, cout]); `extra`: arrays added to S (bias, addend, resid:
    anything that broadcasts to the output)."""
    from oracle import pfnl_spec
    ax, ak = np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(k, np.float64))
    S = pfnl_spec.conv2d_same(ax, ak, None)
    fx, fk = (ax < FLOOR_BELOW).astype(np.float64), (ak < FLOOR_BELOW).astype(np.float64)
    A = pfnl_spec.conv2d_same(ax, fk, None) + pfnl_spec.conv2d_same(fx, ak, None)
    for e in extra:
        if e is not None:
            S = S + np.abs(np.asarray(e, np.float64))
    return S, A


def conv_bound(x, k, extra=(), xerr=None, beta=BETA):
    """Element-wise bound alpha(K) S + beta A for conv2d_same(x, k) [+ extra]; xerr: an element-wise bound on an error the input
    already carries (a fused producer's output), propagated as conv2d_same(xerr, |k|)."""
    from oracle import pfnl_spec
    K = k.shape[0] * k.shape[1] * k.shape[2]
    S, A = conv_terms(x, k, extra)
    b = alpha(K) * S + beta * A
    if xerr is not None:
        b = b + pfnl_spec.conv2d_same(np.asarray(xerr, np.float64), np.abs(np.asarray(k, np.float64)), None)
    return b


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the elements (an element with bound 0 must be exact: ratio inf otherwise)."""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max()) if r.size else 0.0


def equivariant_scales(x, ks=range(-40, 41)):
    """The k of `ks` for which the split commutes with the scale 2^k bit for bit on every element of x:
    hi(2^k x) = 2^k hi(x) and lo'(2^k x) = 2^k lo'(x) (both exactly, 2^k x itself exact in fp32)."""
    x = np.asarray(x, np.float32)
    h0, l0 = (p.astype(np.float64) for p in split_parts(x))
    out = []
    for k in ks:
        xs = (x.astype(np.float64) * 2.0 ** k)
        if not np.array_equal(xs.astype(np.float32).astype(np.float64), xs):
            continue
        h, l = (p.astype(np.float64) for p in split_parts(xs.astype(np.float32)))
        if np.array_equal(h, h0 * 2.0 ** k) and np.array_equal(l, l0 * 2.0 ** k):
            out.append(int(k))
    return out


# ---- data families of the split-f16 op tests -------------------------------------------------------------------------------------

def binades(rng, shape, lo=-30, hi=14, spread=True):
    """+-2^u (1 + v), u uniform over [lo, hi], v uniform [0, 1); channel c (last axis) scaled by 2^((c % 9) - 4) when `spread`;
    |x| < 2^15 (inside binary16's 65504)."""
    u = rng.integers(lo, hi + 1, size=shape).astype(np.float64)
    x = np.ldexp(1.0 + rng.random(shape), u.astype(np.int64)) * rng.choice([-1.0, 1.0], size=shape)
    if spread:
        x = x * 2.0 ** ((np.arange(shape[-1]) % 9) - 4)
    x = np.clip(x, -(2.0 ** 15) * (1 - 2.0 ** -20), 2.0 ** 15 * (1 - 2.0 ** -20))
    return x.astype(np.float32)


def edge_values():
    """fp32 values at the split's edges: +-0, binary16 ties, just below powers of two (hi rounds up a binade, lo' < 0), subnormal hi,
    hi = 0, the top of the 65504 domain."""
    f = np.float32
    v = [0.0, -0.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(1.0 + 2.0 ** -11), 2.0 ** -3 * (1 + 2.0 ** -11),
         np.nextafter(f(1.0), f(0)), np.nextafter(f(2.0 ** -14), f(0)), np.nextafter(f(2.0 ** 10), f(0)), -np.nextafter(f(0.5), f(0)),
         2.0 ** -14, 2.0 ** -15 * 1.3, 2.0 ** -20 * 1.7, 2.0 ** -24, 2.0 ** -24 * 1.5, 2.0 ** -25 * 0.99, 2.0 ** -30, 2.0 ** -36,
         np.nextafter(f(2.0 ** -24), f(1)), 2.0 ** -24 * 2.5, 6.5e4, -6.5e4, 65000.123, 4097.0 + 2.0 ** -11]
    return np.array(v, dtype=np.float32)


def edges(rng, shape):
    """Data made of edge_values() (random positions and signs) mixed with binades: every edge meets every tap position."""
    x = binades(rng, shape, spread=False)
    e = edge_values()
    pick = rng.random(shape) < 0.5
    x[pick] = e[rng.integers(0, e.size, size=int(pick.sum()))] * rng.choice([-1.0, 1.0], size=int(pick.sum())).astype(np.float32)
    return x


def edge_weights(rng, shape, big=6.0e4):
    """Weights from 1e-7 to ~1 (log-uniform, random sign), output channel 0 all zero, one weight near 6e4 (under 65504).
    big=1e6 is the strict-fp32 variant: a weight beyond binary16, which sends the forward to the f32 kernels."""
    w = (10.0 ** rng.uniform(-7, 0, size=shape)) * rng.choice([-1.0, 1.0], size=shape)
    w[..., 0] = 0.0
    w.reshape(-1, shape[-1])[0, 1] = big
    return w.astype(np.float32)


def dark(rng, shape, scale):
    """N(0, 1) data scaled by `scale` (2^-16, 2^-20: where the split's operand floor shows)."""
    return (rng.normal(size=shape) * scale).astype(np.float32)


def unit_binades(rng, shape):
    """|x| in [1/4, 4): the data of the bit-exact scale-equivariance checks (equivariant_scales: k in [-10, 13])."""
    return (np.ldexp(1.0 + rng.random(shape), rng.integers(-2, 2, size=shape)) * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)


def bright(rng, shape, lo=10, hi=40):
    """+-2^u (1 + v), u uniform over [lo, hi] = [10, 40]: nearly every element beyond 65504, where only the strict-fp32 kernels run."""
    u = rng.integers(lo, hi + 1, size=shape)
    return (np.ldexp(1.0 + rng.random(shape), u) * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)


# ---- the Winograd F(2x2,3x3) model of the strict-fp32 3x3 kernels (module docstring) ------------------------------------------

WINO_BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64)
WINO_G = np.array([[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]], np.float64)
WINO_AT = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64)


def alpha_wino(K, epilogue=2):
    """Error per unit of S_w: 2^-24 (sqrt(K) + 2 [input transform] + 1 [U] + 4 [output transform] + epilogue roundings)."""
    return 2.0 ** -24 * (np.sqrt(K) + 7 + epilogue)


def wino_tiles(x, zero_halo=True):
    """The 4x4 input tiles of x [B, H, W, C] (even H, W; zero padding): d[i, j, b, ty, tx, c] = x_padded[b, 2 ty + i, 2 tx + j, c].
    zero_halo=False is a fault for the host test's mutant: the halo column right of the image holds the image's last column."""
    B, H, W, C = x.shape
    assert H % 2 == 0 and W % 2 == 0, "F(2x2,3x3) tiles need even H and W"
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)))
    if not zero_halo:
        xp[:, :, W + 1] = xp[:, :, W]
    return np.stack([np.stack([xp[:, i:i + H:2, j:j + W:2] for j in range(4)]) for i in range(4)])


def wino_u(k):
    """U = G g G^T of HWIO k [3, 3, C, cout] in fp64: [4, 4, C, cout]."""
    return np.einsum("xa,nb,abco->xnco", WINO_G, WINO_G, np.asarray(k, np.float64))


def _untile(y):
    """[2, 2, B, th, tw, cout] -> [B, 2 th, 2 tw, cout]."""
    _, _, B, th, tw, co = y.shape
    return y.transpose(2, 3, 0, 4, 1, 5).reshape(B, 2 * th, 2 * tw, co)


def wino_conv_f64(x, k):
    """The algorithm carried out in fp64 (nothing rounded, U included): equals pfnl_spec.conv2d_same(x, k, None)."""
    d = wino_tiles(np.asarray(x, np.float64))
    V = np.einsum("xi,nj,ijbtuc->xnbtuc", WINO_BT, WINO_BT, d)
    M = np.einsum("xnbtuc,xnco->xnbtuo", V, wino_u(k))
    return _untile(np.einsum("px,qn,xnbtuo->pqbtuo", WINO_AT, WINO_AT, M))


def wino_terms(x, k, extra=()):
    """S_w of the Winograd bound for conv2d_same(x, k) (fp64, [B, H, W, cout]); `extra`: arrays added by magnitude (bias, addend, resid)."""
    d = np.abs(wino_tiles(np.asarray(x, np.float64)))
    U = np.abs(wino_u(k).astype(np.float32).astype(np.float64))
    aB, aA = np.abs(WINO_BT), np.abs(WINO_AT)
    V = np.einsum("xi,nj,ijbtuc->xnbtuc", aB, aB, d)
    M = np.einsum("xnbtuc,xnco->xnbtuo", V, U)
    S = _untile(np.einsum("px,qn,xnbtuo->pqbtuo", aA, aA, M))
    for e in extra:
        if e is not None:
            S = S + np.abs(np.asarray(e, np.float64))
    return S


def _lrelu_f32(o):
    return np.maximum(o, o * np.float32(0.2))


def wino_emulate_f32(x, k, bias=None, addend=None, resid=None, act=True, base=None, base_div=1, per_tile=False, fault=None):
    """numpy fp32 emulation of the Winograd kernels, their order of operations (test infrastructure; the product never imports it).

    x [B, H, W, C] and k [3, 3, C, cout]: C = 64 (modes 0 and 1) or 64 T, the concat of a clip's frames (mode 3: one accumulator over
    all of them).  base [B / base_div, H, W, 64] (one per clip of base_div frames) selects mode 2: k is [3, 3, 128, cout], rows 0..63 the base
    half, whose raw result is finished, kept as an fp32 value and added in the epilogue of each of the clip's frames.  addend / resid broadcast to the output.
      - input transform in fp32: over the rows first (d0 - d2, d1 + d2, d1 - d2 [with -U], d1 - d3), then over the columns;
      - U = fp32(G g G^T) from fp64;
      - one sequential fp32 chain over the channels per (xi, nu), every product formed exactly (an FMA: the sum is formed in fp64
        and rounded once - a double rounding only where the fp64 sum is inexact and lands on an fp32 tie);
      - output transform over nu, then over xi: (m0 + m1) + m2 and m1 - (m2 + m3), or (m1 - m2) - m3 with per_tile (conv_wino.hip);
      - epilogue: + bias, + addend (or + the base partial), max(o, 0.2f o), + resid.
    fault (the host test's mutants): "halo" - the halo column right of the image is not zero; "resid_first" - the residual is added
    before the activation."""
    f = np.float32
    x = np.asarray(x, f)
    if base is not None:
        kb, k = k[:, :, :64], k[:, :, 64:]
        part = np.repeat(_wino_raw_f32(base, kb, per_tile, fault), base_div, axis=0)
    y = _wino_raw_f32(x, k, per_tile, fault)
    o = y + (np.zeros(y.shape[-1], f) if bias is None else np.asarray(bias, f))
    if base is not None:
        o = o + part
    elif addend is not None:
        o = o + np.asarray(addend, f)
    if fault == "resid_first" and resid is not None:
        o = o + np.asarray(resid, f)
    if act:
        o = _lrelu_f32(o)
    if fault != "resid_first" and resid is not None:
        o = o + np.asarray(resid, f)
    return o


def _wino_raw_f32(x, k, per_tile, fault):
    """The transformed convolution itself (no epilogue), fp32 [B, H, W, cout]."""
    f = np.float32
    d = wino_tiles(np.asarray(x, f), zero_halo=fault != "halo")
    t = np.stack([d[0] - d[2], d[1] + d[2], d[1] - d[2], d[1] - d[3]])                       # rows: [xi, j, ...]
    V = np.stack([t[:, 0] - t[:, 2], t[:, 1] + t[:, 2], t[:, 2] - t[:, 1], t[:, 1] - t[:, 3]], axis=1)   # [xi, nu, b, ty, tx, c]
    U = wino_u(k).astype(f)
    U[2] = -U[2]                                                                              # row 2 is d1 - d2
    C = x.shape[-1]
    V64, U64 = V.astype(np.float64), U.astype(np.float64)
    acc = np.zeros(V.shape[:-1] + (U.shape[-1],), f)
    for c in range(C):
        acc = (acc.astype(np.float64) + V64[..., c, None] * U64[:, :, None, None, None, c, :]).astype(f)
    if per_tile:
        s = np.stack([(acc[:, 0] + acc[:, 1]) + acc[:, 2], (acc[:, 1] - acc[:, 2]) - acc[:, 3]])      # [q, xi, ...]
        y = np.stack([(s[:, 0] + s[:, 1]) + s[:, 2], (s[:, 1] - s[:, 2]) - s[:, 3]])                  # [p, q, ...]
    else:
        s = np.stack([(acc[:, 0] + acc[:, 1]) + acc[:, 2], acc[:, 1] - (acc[:, 2] + acc[:, 3])])
        y = np.stack([(s[:, 0] + s[:, 1]) + s[:, 2], s[:, 1] - (s[:, 2] + s[:, 3])])
    return _untile(y)


# ---- the bf16 model of the precision=bf16 kernels (module docstring) ----------------------------------------------------------

def bf16_round(x):
    """fp32 -> the fp32 value of its nearest-even bf16: bf16_rne of conv_bf16.hip bit for bit (NaN stays NaN)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = (u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000
    r = np.where((u & 0x7fffffff) > 0x7f800000, (u | 0x400000) & 0xffff0000, r)
    return r.astype(np.uint32).view(np.float32).reshape(x.shape)


def bf16_trunc(x):
    """fp32 -> bf16 by dropping the low 16 bits (a fault of the host test's mutants)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    return (x.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32).reshape(x.shape)


def bf16_round_away(x):
    """fp32 -> bf16, ties away from zero (a fault of the host test's mutants)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    return ((u + 0x8000) & 0xffff0000).astype(np.uint32).view(np.float32).reshape(x.shape)


def bf16_round64(r):
    """fp64 -> the nearest-even bf16 (as fp32) in ONE rounding: 8 significant bits above 2^-126, the step 2^-133 below; a value just
    off a bf16 tie does not collapse onto the tie in fp32 first.  Beyond bf16's largest finite value: infinity."""
    r = np.asarray(r, np.float64)
    _, ex = np.frexp(r)                                             # |r| = m 2^ex, m in [0.5, 1)
    q = np.maximum(ex.astype(np.int64) - 8, -133)
    with np.errstate(over="ignore"):
        return np.ldexp(np.rint(np.ldexp(r, -q)), q).astype(np.float32)


def bf16_bits(x):
    """The 16-bit patterns of an array of bf16-representable fp32 values."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    assert not (x.view(np.uint32) & np.uint32(0xffff)).any(), "not bf16 values"
    return (x.view(np.uint32) >> np.uint32(16)).astype(np.uint16).reshape(x.shape)


def bf16_slack(K, n_e, S):
    """e = (alpha(K) + n_e 2^-24) S: the distance of the fp32 value in front of the store from the fp64 result (module docstring)."""
    return (alpha(K) + n_e * 2.0 ** -24) * np.asarray(S, np.float64)


def bf16_interval(r, e):
    """(lo, hi) = (bf16(r - e), bf16(r + e)), one rounding each: a correct kernel's output lies in [lo, hi] element-wise."""
    r, e = np.asarray(r, np.float64), np.asarray(e, np.float64)
    return bf16_round64(r - e), bf16_round64(r + e)


def bf16_pinned(lo, hi):
    """The elements whose interval admits one bf16 value only (the test is bit-exact there)."""
    return lo == hi


def bf16_outside(got, lo, hi):
    """The elements of got outside [lo, hi]."""
    got = np.asarray(got, np.float32)
    return ~((lo <= got) & (got <= hi))


def _bf16_neighbours(g):
    """The bf16 numbers just below and just above every element of g (bf16 values as fp32), in fp64."""
    b = bf16_bits(g).astype(np.int64)
    k = np.where(b < 0x8000, b, -(b & 0x7fff))                      # ordered integers; +-0 -> 0
    def val(k):
        bits = np.where(k >= 0, k, 0x8000 | -k).astype(np.uint32) << np.uint32(16)
        return bits.view(np.float32).astype(np.float64)
    return val(k - 1), val(k + 1)


def bf16_smallest_factor(got, r, e):
    """The smallest c for which bf16_interval(r, c e) admits every element of got (bf16 values): per element the distance of r from
    the rounding cell of got, in units of e (0 where got is the rounding of r itself; inf where e = 0 and it is not)."""
    g = np.asarray(got, np.float32)
    r, e = np.asarray(r, np.float64), np.asarray(e, np.float64)
    below, above = _bf16_neighbours(g)
    g64 = g.astype(np.float64)
    d = np.maximum(np.maximum((g64 + below) / 2 - r, r - (g64 + above) / 2), 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(d == 0, 0.0, d / e)
    return float(c.max()) if c.size else 0.0


def bf16_spec(x, k, bias=None, addend=None, add_div=1, resid=None, act=True, n_e=None):
    """(r, e) of one bf16 launch: the fp64 spec act(conv2d_same(x, bf16_round(k)) + bias + addend[item / add_div]) + resid on the bf16
    inputs, and the slack (alpha(K) + n_e 2^-24) S.  x [items, H, W, C] (for the 1x1 and convmerge1: the concat over the frames);
    n_e: 4 with an addend, else 2, unless given."""
    from oracle import pfnl_spec
    f64 = lambda a: None if a is None else np.asarray(a, np.float64)          # noqa: E731
    kr = bf16_round(k)
    y = pfnl_spec.conv2d_same(f64(x), f64(kr), f64(bias))
    add = None if addend is None else np.repeat(f64(addend), add_div, axis=0)
    if add is not None:
        y = y + add
    if act:
        y = pfnl_spec.lrelu(y)
    if resid is not None:
        y = y + f64(resid)
    S, _ = conv_terms(x, kr, (bias, add, resid))
    if n_e is None:
        n_e = 4 if addend is not None else 2
    return y, bf16_slack(k.shape[0] * k.shape[1] * k.shape[2], n_e, S)


def concat_frames(x, T):
    """[clips T, H, W, 64] -> [clips, H, W, 64 T]: the reference's concat over the frames of a clip."""
    F, H, W, c = x.shape
    return x.reshape(F // T, T, H, W, c).transpose(0, 2, 3, 1, 4).reshape(F // T, H, W, T * c)


# data families of the bf16 tests: activations are bf16 values; weights are NOT pre-rounded (the hooks round them, the spec with bf16_round)

BF16_FAMILIES = ["normal", "binades", "bright", "dark16", "dark20", "bf16_edges"]


def bf16_edges(rng, shape, lo=-120, hi=120):
    """bf16 values at the format's edges: +-(s 2^-7) 2^u with 8-bit significands s in [128, 256) - half of them drawn from
    255 (0x..7f: just below a power of two), 128, 129 / 253 (odd), 130 / 254 (even) - and u uniform over [lo, hi), 3 % zeros of either
    sign, channel 5 (last axis) all zero.  Channel 0 stays below 2^(hi - 30): edge_weights(big=1e6) puts its large weight there and
    results beyond bf16's largest finite value are not this test's subject."""
    s = rng.integers(128, 256, size=shape)
    pick = rng.random(shape) < 0.5
    s[pick] = np.array([255, 128, 129, 253, 130, 254])[rng.integers(0, 6, size=int(pick.sum()))]
    u = rng.integers(lo, hi, size=shape)
    u[..., 0] = np.minimum(u[..., 0], hi - 30)
    x = np.ldexp(s.astype(np.float64), u - 7) * rng.choice([-1.0, 1.0], size=shape)
    x[rng.random(shape) < 0.03] = 0.0
    x = x.astype(np.float32)
    neg0 = rng.random(shape) < 0.5
    x[(x == 0) & neg0] = -0.0
    if shape[-1] > 5:
        x[..., 5] = 0.0
    return x


def bf16_xdata(rng, fam, shape, hi=120):
    """Activations of a bf16 family (bf16 values as fp32)."""
    if fam == "normal":
        return bf16_round(rng.normal(size=shape).astype(np.float32))
    if fam == "binades":
        return bf16_round(binades(rng, shape))
    if fam == "bright":
        return bf16_round(bright(rng, shape))
    if fam == "bf16_edges":
        return bf16_edges(rng, shape, hi=hi)
    return bf16_round(dark(rng, shape, 2.0 ** -int(fam[4:])))


def bf16_wdata(rng, fam, shape):
    """Weights of a bf16 family, fp32 and not rounded: N(0, 1 / fan-in); bf16_edges: edge_weights with big=1e6."""
    if fam == "bf16_edges":
        return edge_weights(rng, shape, big=1.0e6)
    return (rng.normal(size=shape) / np.sqrt(np.prod(shape[:-1]))).astype(np.float32)


def bf16_bias(rng, fam, n):
    """A bias at the family's scale, fp32 (the kernels take it unrounded); element 0 is zero.  normal: N(0, 1), as large as the
    convolution itself - a zero-mean output passes through zero, where the slack spans many bf16 steps and the interval pins nothing;
    the bias thins those outputs out (pinned share of the plain launch 0.90 with a bias of 0.1, the floor the tests hold the data to)."""
    scale = {"dark16": 2.0 ** -18, "dark20": 2.0 ** -22, "bright": 2.0 ** 20, "normal": 1.0}.get(fam, 0.1)
    b = (rng.normal(size=n) * scale).astype(np.float32)
    b[0] = 0.0
    return b


def identity_kernel():
    """HWIO [3, 3, 64, 64]: the centre tap is the identity, weight 1."""
    k = np.zeros((3, 3, 64, 64), np.float32)
    k[1, 1, np.arange(64), np.arange(64)] = 1.0
    return k


def bf16_ties_plain(rng, shape, elo=-20, ehi=20):
    """(x, bias, want) of the plain identity launch with the activation off: channel c holds +-(s 2^-7) 2^E_c with random 8-bit
    significands s, the bias is +-2^(E_c - 8) in fp32, so x + bias is exact in fp32 and lies exactly between two bf16 numbers (on
    one where the signs differ and s = 128); want = bf16_round(x + bias)."""
    C = shape[-1]
    E = rng.integers(elo, ehi + 1, size=C)
    x = (np.ldexp(rng.integers(128, 256, size=shape).astype(np.float64), E - 7) * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)
    bias = (np.ldexp(1.0, E - 8) * rng.choice([-1.0, 1.0], size=C)).astype(np.float32)
    r = x.astype(np.float64) + bias.astype(np.float64)
    assert np.array_equal((x + bias).astype(np.float64), r)                  # exact in fp32
    return x, bias, bf16_round(x + bias)


def bf16_ties_fused(rng, clips, T, H, W, elo=-20, ehi=20):
    """(addend, resid, want) of the fused launch with zero weights and zero bias: the addend a = (s 2^-7) 2^E > 0 with E drawn per
    element of the clip, resid = 2^(E - 8) for each of its frames; act(0 + 0 + a) + resid = a + resid exactly, a bf16 tie."""
    E = rng.integers(elo, ehi + 1, size=(clips, H, W, 64))
    a = np.ldexp(rng.integers(128, 256, size=E.shape).astype(np.float64), E - 7).astype(np.float32)
    resid = np.repeat(np.ldexp(1.0, E - 8).astype(np.float32), T, axis=0)
    s = np.repeat(a, T, axis=0) + resid
    assert np.array_equal(s.astype(np.float64), np.repeat(a, T, axis=0).astype(np.float64) + resid.astype(np.float64))
    return a, resid, bf16_round(s)


def identity_inputs(rng, shape):
    """bf16 values over 60 binades with zeros of both signs among them, and what the zero-bias identity launch returns for them:
    the input bit for bit, -0 as +0 (module docstring)."""
    x = (np.ldexp(rng.integers(128, 256, size=shape).astype(np.float64), rng.integers(-37, 23, size=shape)) *
         rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)
    z = rng.random(shape) < 0.05
    x[z] = np.where(rng.random(int(z.sum())) < 0.5, np.float32(-0.0), np.float32(0.0))
    return x, x + np.float32(0.0)


BF16_FAULTS = ("trunc_store", "half_away", "round_before_resid", "trunc_weights", "c10_unrounded", "addend_mod", "resid_first")


def _chain_f32(x, k):
    """conv2d_same(x, k) as ONE sequential fp32 chain per output over (ky, kx, ci), every product formed exactly (bf16 operands: the
    sum is formed in fp64 and rounded once to fp32); the accumulator starts from +0."""
    f = np.float32
    ks = k.shape[0]
    p = ks // 2
    B, H, W, C = x.shape
    xp = np.pad(np.asarray(x, np.float64), ((0, 0), (p, p), (p, p), (0, 0)))
    k64 = np.asarray(k, np.float64)
    acc = np.zeros((B, H, W, k.shape[-1]), f)
    for ky in range(ks):
        for kx in range(ks):
            win = xp[:, ky:ky + H, kx:kx + W]
            for c in range(C):
                acc = (acc.astype(np.float64) + win[..., c, None] * k64[ky, kx, c]).astype(f)
    return acc


def bf16_emulate(x, k, bias=None, addend=None, add_div=1, resid=None, act=True, k10=None, b10=None, T=1, out_f32=False, fault=None):
    """numpy fp32 restatement of the bf16 kernels' rounding points (test infrastructure; the product never imports it).

    x [items, H, W, C] bf16 values (for the 1x1 and convmerge1: the concat over the frames), k fp32 HWIO, rounded here as the hooks
    round it.  Sequential fp32 chain with exact products; epilogue + bias, + addend[item / add_div], max(o, 0.2f o), + resid; one
    nearest-even store (none with out_f32: convmerge1).  (The 3x3 kernels start the accumulator from the bias instead of adding it last:
    another order of the same fp32 additions, inside the same slack.)  k10 / b10 / T: conv1_i + conv10_i, returns (out1, base) with base the
    same restatement of the 1x1 over the ROUNDED out1.
    fault (BF16_FAULTS, the host test's mutants): trunc_store - the store truncates; half_away - it rounds ties away from zero;
    round_before_resid - the activation's result is rounded to bf16, then + resid, then rounded again; trunc_weights - the pack
    truncates; c10_unrounded - conv10_i reads the fp32 out1; addend_mod - the addend of item % add_div; resid_first - the residual
    goes in before the activation."""
    f = np.float32
    assert fault is None or fault in BF16_FAULTS, fault
    store = {"trunc_store": bf16_trunc, "half_away": bf16_round_away}.get(fault, bf16_round)
    wround = bf16_trunc if fault == "trunc_weights" else bf16_round
    o = _chain_f32(x, wround(k))
    if bias is not None:
        o = o + np.asarray(bias, f)
    if addend is not None:
        item = np.arange(x.shape[0])
        o = o + np.asarray(addend, f)[(item % add_div) % len(addend) if fault == "addend_mod" else item // add_div]
    if fault == "resid_first" and resid is not None:
        o = o + np.asarray(resid, f)
    if act:
        o = _lrelu_f32(o)
    if resid is not None and fault != "resid_first":
        if fault == "round_before_resid":
            o = bf16_round(o)
        o = o + np.asarray(resid, f)
    out = o if out_f32 else store(o)
    if k10 is None:
        return out
    b = _chain_f32(concat_frames(o if fault == "c10_unrounded" else out, T), wround(k10))
    if b10 is not None:
        b = b + np.asarray(b10, f)
    return out, store(_lrelu_f32(b))


BF16_MODES = ("plain", "fused", "c1c10", "1x1", "merge")


def bf16_case(mode, fam, rng, clips, T, H, W, cout=64):
    """The inputs of one bf16 launch on one family, as keyword arguments of bf16_emulate (x per frame: [clips T, H, W, 64]; the 1x1
    and convmerge1 take concat_frames(x, T)).  c1c10 on bf16_edges keeps its inputs under 2^100: out1 feeds a second sum."""
    F = clips * T
    x = bf16_xdata(rng, fam, (F, H, W, 64), hi=100 if mode == "c1c10" else 120)
    if mode == "1x1":
        return dict(x=x, k=bf16_wdata(rng, fam, (1, 1, 64 * T, 64)), bias=bf16_bias(rng, fam, 64))
    if mode == "merge":
        return dict(x=x, k=bf16_wdata(rng, fam, (3, 3, 64 * T, cout)), bias=bf16_bias(rng, fam, cout))
    kw = dict(x=x, k=bf16_wdata(rng, fam, (3, 3, 64, 64)), bias=bf16_bias(rng, fam, 64))
    if mode == "fused":
        kw.update(addend=bf16_xdata(rng, fam, (clips, H, W, 64)), add_div=T, resid=bf16_xdata(rng, fam, (F, H, W, 64)))
    if mode == "c1c10":
        kw.update(k10=bf16_wdata(rng, fam, (1, 1, 64 * T, 64)), b10=bf16_bias(rng, fam, 64), T=T)
    return kw


def bf16_report(got, r, e):
    """(share outside [lo, hi], pinned share, pinned elements, pinned elements that match, smallest factor c) of a bf16 output."""
    lo, hi = bf16_interval(r, e)
    pin = bf16_pinned(lo, hi)
    got = np.asarray(got, np.float32)
    return (float(bf16_outside(got, lo, hi).mean()), float(pin.mean()), int(pin.sum()), int((pin & (got == lo)).sum()),
            bf16_smallest_factor(got, r, e))
