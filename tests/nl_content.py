"""Image-like content for the non-local kernels, a closed-form fp64 reference for palette clips, and the error bound the long-chain
tests hold the three attention kernels to (host only: numpy, no device).

CONTENT.  The model's real input is u8 / 255 in fp32: exact zeros and ones, large flat regions, dark frames, ramps, a few dominant
pixels.  `levels8` draws such frames; `palette_clip` builds a clip whose space-to-depth cells (the keys, queries and values of the
block: C = 12 T channels each) come from a palette of k entries, placed by an `index_grid` in the key order the kernels walk
(row-major over the H/2 x W/2 grid).  Flat frames, two-tone frames, ramps and "one bright cell" are palettes with different grids.

THE CLOSED FORM.  A clip of k palette entries v_1..v_k with counts n_b gives a query of entry a

    mean_a = sum_b n_b e^{v_a.v_b} v_b / sum_b n_b e^{v_a.v_b},        out_a = v_a + (mean_a Wg + bg) Ww + bw

(rows of the softmax sum to 1, so g's bias passes through): O(k^2 C) in fp64 whatever N is.  `class_reference` subtracts the row
maximum first, as pfnl_spec.nonlocal_block(stabilise=True) does.

THE BOUND (`attention_bound`), element-wise against that fp64 reference, in the style of tests/numerics.py.  With the normalised
weights p_j of a query (sum 1), u = 2^-24 and, per channel,

    mean = sum_j p_j v_j,      A = sum_j p_j |v_j|,      D = sum_j p_j |v_j - mean|   (the spread: 0 on flat content)

the kernels' mean is off by at most

    E = u U A  +  (e^{2 eps} - 1) D  +  val A + floor  +  (4 + ks) u A                                                    (*)

  - u U A: sum_j p_j v_j is ONE fp32 accumulator per lane, updated U times along the longest chain of keys one workgroup walks
    (keys per key split): U = keys / 2 on the f32 pipe (v_mfma_f32_32x32x2_f32: two keys per instruction) and keys / 16 on the f16
    pipe (v_mfma_f32_32x32x16_f16: sixteen exact products, then the accumulator).  Every update rounds the running sum, by at most
    u |partial| <= u sum_j p_j |v_j| (before the normalisation).  This is the deterministic worst case, NOT numerics.alpha's
    sqrt(K): on a flat region every addend is equal, the rounding error keeps ONE sign for a whole binade of the accumulator and
    grows linearly in the chain length.  (The f32 MFMA rounds after each of its two products - it is an fmaf chain bit for bit - and
    the split kernel feeds an accumulator three MFMAs per 16 keys: counted per rounding the chains are 2 x and up to 3 x longer.
    The term still covers them wherever the partial sums grow with the keys, as on flat and two-tone content: the k-th of n
    roundings is then at most u (k / n) of the total, n / 2 of them in all.)
  - (e^{2 eps} - 1) D: an error eps_j in the (natural) logit of key j turns p_j into p_j e^{eps_j}; as sum_j p_j (v_j - mean) = 0,
    the mean moves by |sum_j p_j (e^{eps_j} - 1)(v_j - mean)| / sum_j p_j e^{eps_j} <= (e^eps - 1) e^eps D <= (e^{2 eps} - 1) D.
    eps = rel L + floor_l + arg, with L = max_j sum_c |q_c k_jc| (the absolute logit mass: the logit itself for an image) and
        f32      rel = (C + 4) u: the query scaled by log2 e (one rounding), a chain of C fmafs, the subtraction of the maximum;
        split16  rel = 3 x 2^-22 + 18 u: K and Q as hi + lo binary16 pairs (2^-22 relative each while lo is a normal number), the
                 dropped lo.lo product (2^-22), 18 accumulator roundings;
        f16      rel = 2 x 2^-11 + 6 u: one binary16 rounding per operand, 6 accumulator roundings.
      floor_l = 2^-32 sum_c (|q_c| + |k_c|) for the f16 pipe: an operand is scaled by 2^7 before it is rounded, and below 2^-14 a
      binary16 step is 2^-24 - half of it, over 2^7, per operand, times its partner.  (Values under 0.001 leave lo there.)
      arg = 2^-22 (f32: v_exp_f32, one ulp) or 2^-20 (f16 pipe: the exponent argument s 2^-14 + 14 - max is one fma, rounded at a
      magnitude of up to 14 for every probability that survives; plus v_exp_f32); on the hi-only kernel also 2^-11 for P itself,
      rounded to binary16 - the row sum accumulates the SAME rounded values, so that is a change of weight, not of mass.
  - val A + floor: the value operand.  f32: exact (0).  split16: 2^-22 A + 2^-32 (V = hi + lo, lo unscaled: exact below 2^-14 only
    down to the 2^-24 step).  f16: 2^-11 A + 2^-32.  On the f16 pipe a probability under 2^-28 of the row maximum is a binary16
    subnormal or zero: at most 2^-39 of the row's mass per key is lost or gained, keys x 2^-39 (v in [0, 1]) - part of `floor`.
  - (4 + ks) u A: 1 / l, O / l, and for ks key splits the merge (nl_merge_kernel: a weight, ks fmafs, one division).

(*) goes through the folded projection W' = Wg Ww as E |W'|, and the output collects

    bound = E |W'|  +  proj (|mean| |W'|)  +  u |b'|  +  3 u (|x| + |z| + |b'|)

  - proj: the projection's own round-off.  f32: (C + 2) u (W' rounded to fp32 on the host, a chain of C fmafs).  f16 pipe (both
    kernels project in split arithmetic): 3 x 2^-22 + 20 u (O and W' as split pairs, the dropped lo.lo, 18 accumulator roundings,
    the two accumulators joined, W' rounded on the host).
  - u |b'|: the folded bias b' = bg Ww + bw, rounded to fp32 on the host.
  - 3 u (...): out = x + z + b' is two fp32 additions (after the merge: a division and two additions).

Nothing in the bound is measured on the kernels: every term is a count of roundings times the unit of its number format."""
import numpy as np

from oracle import pfnl_spec

U32 = 2.0 ** -24                    # unit round-off of fp32 (half an ulp, relative)
KERNELS = ("fp32", "split16", "f16")
FLAT_TOL = {"fp32": 2e-5, "split16": 2e-5, "f16": 2e-3}     # the suite's tolerances for |x| <= 1 (tests/test_gpu_ops.py)
NL_KT = 64                          # keys per LDS tile (nonlocal.hip NL_KT, nonlocal_f16.hip NF_KT)


# ---- generators: x [B, T, H, W, 3] float32 inside [0, 1] ---------------------------------------------------------------------------

def dequant8(u8):
    """u8 / 255. in fp32, as the streaming session's table dequantises (pfnl_amd/stream.py)."""
    return (np.asarray(u8, dtype=np.uint8) / 255.).astype(np.float32)


def levels8(rng, shape, lo=0, hi=255):
    """Frames of 8-bit levels lo..hi (inclusive), uniform."""
    return dequant8(rng.integers(lo, hi + 1, size=shape, dtype=np.int64).astype(np.uint8))


def dark8(rng, shape):
    """Levels 0..3, at least a third of the samples exactly 0 (a dark frame with letterbox-black pixels)."""
    u = rng.integers(0, 4, size=shape)
    u[rng.random(shape) < 1.0 / 3.0] = 0
    return dequant8(u.astype(np.uint8))


PRESETS = {
    "full": lambda rng, shape: levels8(rng, shape, 0, 255),
    "dark": dark8,
    "saturated": lambda rng, shape: levels8(rng, shape, 252, 255),
    "zeros": lambda rng, shape: dequant8(np.zeros(shape, np.uint8)),
    "ones": lambda rng, shape: dequant8(np.full(shape, 255, np.uint8)),
}


def sub_milli(rng, shape):
    """Floats in (0, 0.001): the lo operand of the 2^7-scaled split is a binary16 subnormal."""
    x = (1e-6 + rng.random(shape) * (0.001 - 2e-6)).astype(np.float32)
    assert x.min() > 0 and x.max() < 0.001
    return x


def cells_of(x):
    """x [B, T, H, W, 3] -> the space-to-depth cells [B, H/2, W/2, 12 T] (the block's keys / queries / values), dtype kept."""
    T = x.shape[1]
    return pfnl_spec.space_to_depth2(np.concatenate([x[:, t] for t in range(T)], -1))


def clip_of(cells_grid):
    """[B, H/2, W/2, 12 T] -> x [B, T, H, W, 3]: the inverse of cells_of."""
    stack = pfnl_spec.depth_to_space2(cells_grid)
    T = stack.shape[-1] // 3
    return np.ascontiguousarray(np.stack([stack[..., 3 * t:3 * t + 3] for t in range(T)], axis=1))


def palette_clip(cells, index_grid):
    """cells [k, C = 12 T] (channel order of pfnl_spec.space_to_depth2 applied to the frame stack), index_grid [B, H/2, W/2] ints:
    the clip x [B, T, H, W, 3] float32 whose grid cell (b, i, j) is cells[index_grid[b, i, j]]."""
    cells = np.asarray(cells, dtype=np.float32)
    assert cells.ndim == 2 and cells.shape[1] % 12 == 0
    return clip_of(cells[np.asarray(index_grid)])


def flat_cells(levels, C):
    """One palette entry per 8-bit level: all C channels at level / 255."""
    return np.repeat(dequant8(np.asarray(levels, np.uint8))[:, None], C, axis=1)


def self_logit(cells):
    c = np.asarray(cells, np.float64)
    return (c * c).sum(-1)


def _spread(order, N):
    """N keys over len(order) palette entries in the given order, as evenly as the counts allow."""
    order = np.asarray(order)
    return order[(np.arange(N) * len(order)) // N]


def ascending(cells, N):
    """Flat index grid [N]: the palette entries by rising self-logit along the key order - the running maximum of every query
    rises whenever a new entry starts."""
    return _spread(np.argsort(self_logit(cells), kind="stable"), N)


def descending(cells, N):
    """... by falling self-logit: the maximum sits in the first half, everything later is rescaled against it."""
    return _spread(np.argsort(self_logit(cells), kind="stable")[::-1], N)


def dominant_at(pos, N, entry=1, other=0):
    """Flat index grid [N]: `entry` at key `pos`, `other` everywhere else."""
    g = np.full(N, other, dtype=np.int64)
    g[pos] = entry
    return g


def split_tile_range(sp, ks, N):
    """Keys [first, last) of key split sp of ks: nonlocal.hip / nonlocal_f16.hip give workgroup z = sp the 64-key tiles
    [ntiles * sp / ks, ntiles * (sp + 1) / ks), ntiles = ceil(N / 64) (kt0 / kt1 in nl_attn_kernel and nl_attn_f16_sw_kernel)."""
    ntiles = (N + NL_KT - 1) // NL_KT
    return min(N, ntiles * sp // ks * NL_KT), min(N, ntiles * (sp + 1) // ks * NL_KT)


def block_in_split(sp, ks, N, entry=1, other=0):
    """Flat index grid [N]: `entry` on exactly the keys of key split sp of ks (split_tile_range), `other` elsewhere."""
    g = np.full(N, other, dtype=np.int64)
    a, b = split_tile_range(sp, ks, N)
    g[a:b] = entry
    return g


def key_splits(B, N):
    """nl_key_splits(B, N) of nonlocal.hip: the key splits of the f32 kernel, and the cap of the f16 kernels' choice."""
    qblocks, ntiles = (N + 127) // 128, (N + NL_KT - 1) // NL_KT
    ks = min(8, (512 + qblocks * B - 1) // (qblocks * B))
    ks = min(ks, ntiles // (4 if qblocks * B >= 32 else 1))
    return max(ks, 1)


def key_splits_f16(B, N):
    """The f16 kernels' choice (nl_attn_f16_run, whole frame): the k <= nl_key_splits that minimises ceil(blocks k / 256) / k."""
    qb = (N + 255) // 256 * B
    best, ks = 1e30, 1
    for k in range(1, key_splits(B, N) + 1):
        t = ((qb * k + 255) // 256) / k
        if t < best - 1e-9:
            best, ks = t, k
    return ks


def longest_chain(N, ks):
    """Keys of the longest chain one workgroup walks with ks key splits."""
    return max(b - a for a, b in (split_tile_range(sp, ks, N) for sp in range(ks)))


# ---- the closed form -------------------------------------------------------------------------------------------------------------------

def class_stats(cells, counts):
    """fp64, per query entry a: P [k, k] (the mass sum_{j in b} p_j of every entry b), mean, A = sum p |v|, D = sum p |v - mean|
    [k, C] each, and L [k] = max_b sum_c |v_ac v_bc| over the entries present."""
    v = np.asarray(cells, np.float64)
    n = np.asarray(counts, np.float64)
    f = v @ v.T
    f = np.where(n[None, :] > 0, f, -np.inf)
    f = f - f.max(axis=1, keepdims=True)                            # stabilise=True
    w = n[None, :] * np.exp(f)
    P = w / w.sum(axis=1, keepdims=True)
    mean = P @ v
    A = P @ np.abs(v)
    D = np.einsum("ab,abc->ac", P, np.abs(v[None, :, :] - mean[:, None, :]))
    L = np.where(n[None, :] > 0, np.abs(v) @ np.abs(v).T, 0.0).max(axis=1)
    return P, mean, A, D, L


def _mats(wg, bg, ww, bw):
    C = np.asarray(bg).size
    f = lambda a, s: np.asarray(a, np.float64).reshape(s)           # noqa: E731
    return f(wg, (C, C)), f(bg, C), f(ww, (C, C)), f(bw, C)


def class_reference(cells, counts, wg, bg, ww, bw):
    """Rows [k, C] in fp64: what pfnl_spec.nonlocal_block(stabilise=True) + the residual of model/pfnl.py:60 give a grid cell of
    palette entry a in a clip that holds counts[b] cells of entry b (module docstring).  `class_expand` places them."""
    wg, bg, ww, bw = _mats(wg, bg, ww, bw)
    _, mean, _, _, _ = class_stats(cells, counts)
    return np.asarray(cells, np.float64) + (mean @ wg + bg) @ ww + bw


def class_expand(rows, index_grid):
    """rows [k, C] placed by index_grid [B, H/2, W/2] -> [B, H, W, 3 T], the layout of ops.nonlocal_residual's output."""
    return pfnl_spec.depth_to_space2(np.asarray(rows)[np.asarray(index_grid)])


# ---- the bound ---------------------------------------------------------------------------------------------------------------------------

def accumulator_updates(kernel, keys):
    """fp32 accumulator updates along a chain of `keys` keys: one per 2 keys on the f32 pipe, one per 16 on the f16 pipe."""
    return -(-int(keys) // (2 if kernel == "fp32" else 16))


def logit_eps(kernel, C, L, qk_abs):
    """eps of the module docstring (natural-log units); qk_abs = sum_c (|q_c| + |k_c|) at its largest over the keys."""
    if kernel == "fp32":
        return (C + 4) * U32 * L + 2.0 ** -22
    if kernel == "split16":
        return (3 * 2.0 ** -22 + 18 * U32) * L + 2.0 ** -32 * qk_abs + 2.0 ** -20
    if kernel == "f16":
        return (2 * 2.0 ** -11 + 6 * U32) * L + 2.0 ** -32 * qk_abs + 2.0 ** -20 + 2.0 ** -11
    raise KeyError(kernel)


def mean_bound(kernel, A, D, L, qk_abs, C, chain_keys, total_keys, ks=1):
    """E of the module docstring: a bound on the error of the attention mean itself (any shape that broadcasts)."""
    eps = logit_eps(kernel, C, L, qk_abs)
    val = {"fp32": 0.0, "split16": 2.0 ** -22, "f16": 2.0 ** -11}[kernel]
    floor = 0.0 if kernel == "fp32" else 2.0 ** -32 + total_keys * 2.0 ** -39
    return U32 * accumulator_updates(kernel, chain_keys) * A + np.expm1(2 * eps) * D + val * A + floor + (4 + ks) * U32 * A


def attention_bound(kernel, cells, counts, wg, bg, ww, bw, chain_keys, ks=1):
    """Rows [k, C]: the element-wise bound on |kernel - class_reference| for a palette clip (module docstring).  chain_keys: the
    longest chain of keys one workgroup walks (longest_chain); ks: the key splits merged."""
    wg, bg, ww, bw = _mats(wg, bg, ww, bw)
    v = np.asarray(cells, np.float64)
    C = v.shape[1]
    n = np.asarray(counts, np.float64)
    _, mean, A, D, L = class_stats(v, n)
    absum = np.abs(v).sum(axis=1)
    qk_abs = absum + absum[n > 0].max()
    E = mean_bound(kernel, A, D, L[:, None], qk_abs[:, None], C, chain_keys, float(n.sum()), ks)
    Wf = np.abs(wg @ ww)
    bf = np.abs(bg @ ww + bw)
    proj = (C + 2) * U32 if kernel == "fp32" else 3 * 2.0 ** -22 + 20 * U32
    z = np.abs(mean @ (wg @ ww))
    return E @ Wf + proj * (np.abs(mean) @ Wf) + U32 * bf + 3 * U32 * (np.abs(v) + z + bf)


# ---- float32 emulations (host tests): what the arithmetic alone does, and what a wrong kernel would do ---------------------------------

def chain_mean_f32(values, weights, per_step):
    """sum_j w_j v_j / sum_j w_j over the keys in order, in ONE float32 accumulator each, `per_step` products per update: the
    products of a step are summed exactly (fp64), then added to the accumulator with one fp32 rounding.  per_step = 1: an fmaf chain,
    one rounding per key (what v_mfma_f32_32x32x2_f32 does bit for bit); 2: one rounding per f32 MFMA; 16: the f16 pipe.
    values [n, C] and weights [n] are taken as float32 numbers (the probabilities and values the kernels hold)."""
    v = np.asarray(values, np.float32).astype(np.float64)
    w = np.asarray(weights, np.float32).astype(np.float64)
    n = v.shape[0]
    pad = -n % per_step
    wv = np.concatenate([w[:, None] * v, np.zeros((pad, v.shape[1]))]).reshape(-1, per_step, v.shape[1]).sum(axis=1)
    ww_ = np.concatenate([w, np.zeros(pad)]).reshape(-1, per_step).sum(axis=1)
    num = np.zeros(v.shape[1], np.float32)
    den = np.float32(0)
    for i in range(wv.shape[0]):
        num = (num.astype(np.float64) + wv[i]).astype(np.float32)
        den = np.float32(np.float64(den) + ww_[i])
    return num.astype(np.float64) / np.float64(den)


def streaming_attention(X, ks=1, half=32, drop_alpha=False, equal_merge=False):
    """The kernels' algorithm in float32 numpy, every query of X [N, C] at once: keys in 32-key halves, a running maximum m per
    query with the o *= alpha rescale, the row sum carried next to o, ks key splits over split_tile_range merged with the weights
    exp2(m_p - m) as nl_merge_kernel does.  Returns the attention mean [N, C] (no projection).
    drop_alpha: leave the rescale out.  equal_merge: merge the parts with weight 1.  (Two wrong kernels the tests must catch.)"""
    X = np.asarray(X, np.float32)
    N, C = X.shape
    f32 = np.float32
    S = (X * f32(1.4426950408889634)) @ X.T                        # base-2 logits [query, key]
    parts = []
    for sp in range(ks):
        a, b = split_tile_range(sp, ks, N)
        m = np.full(N, -np.inf, f32)
        o = np.zeros((N, C), f32)
        l = np.zeros(N, f32)
        for h0 in range(a, b, half):
            s = S[:, h0:min(h0 + half, b)]
            mn = np.maximum(m, s.max(axis=1))
            alpha = np.exp2(m - mn).astype(f32)
            p = np.exp2(s - mn[:, None]).astype(f32)
            if not drop_alpha:
                o, l = o * alpha[:, None], l * alpha
            o = o + p @ X[h0:h0 + s.shape[1]]
            l = l + p.sum(axis=1)
            m = mn
        parts.append((m, l, o))
    if ks == 1:
        return o / l[:, None]
    m = np.max([p[0] for p in parts], axis=0)
    num, den = np.zeros((N, C), f32), np.zeros(N, f32)
    for mp, lp, op in parts:
        w = np.ones(N, f32) if equal_merge else np.exp2(mp - m).astype(f32)
        num, den = num + w[:, None] * op, den + w * lp
    return num / den[:, None]
