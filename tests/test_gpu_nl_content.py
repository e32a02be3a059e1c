"""The non-local kernels on image-like content and long key chains (tests/nl_content.py has the generators, the closed-form
reference and the bound).

Every case runs through ops.nonlocal_residual on the three attention kernels - nl_attn_kernel (f32 MFMA, "fp32"),
nl_attn_f16_sw_kernel<C, true> ("split16") and <C, false> ("f16") - with their pack, merge and projection stages:
  a. 8-bit levels (full range, dark, saturated, all zero, all one) and values under 0.001 at one tile, a partial last half and the
     key-split path, against the fp64 spec; zeros and ones also as closed forms; sub-milli values through ops.nonlocal_block
     (pool and q-projection kernels);
  b. the identity projection with one dominant key at the first key, the end of a full tile, the last real key of a partial half
     and the first key of the last tile: out - x is that key's value to the precision of the value operand;
  c. running maxima that rise at every 32-key half or sit in the first one, through a ring that turns more than once and through 8
     key splits; key splits whose parts differ by 2^121 in weight;
  d. flat and two-tone frames over unsplit chains of 4096 and 16384 keys and over 4 merged chains, against the closed form and the
     derived bound of nl_content (not the flat tolerance: the drift of an fp32 accumulator on equal addends is linear in the chain);
  e. flat frames at non-dyadic levels at 16 x 16.
Each test prints its worst error or bound ratio (-s)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import nl_content as NC  # noqa: E402
from numerics import worst_ratio  # noqa: E402
from oracle import pfnl_spec  # noqa: E402
from pfnl_amd import ops  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
KERNELS = NC.KERNELS
TOL = NC.FLAT_TOL

_cache = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _weights(seed, C):
    if ("w", seed, C) not in _cache:
        rng = np.random.default_rng(seed)
        wg = (rng.normal(size=(1, 1, C, C)) / np.sqrt(C)).astype(np.float32)
        ww = (rng.normal(size=(1, 1, C, C)) / np.sqrt(C)).astype(np.float32)
        _cache["w", seed, C] = (wg, rng.normal(size=C).astype(np.float32) * 0.1, ww, rng.normal(size=C).astype(np.float32) * 0.1)
    return _cache["w", seed, C]


def _identity(C):
    eye = np.eye(C, dtype=np.float32).reshape(1, 1, C, C)
    return eye, np.zeros(C, np.float32), eye, np.zeros(C, np.float32)


def _spec(key, x, w):
    """stack + NonLocalBlock in fp64 with stabilise=True, computed once per `key` (shared by the three kernels)."""
    if ("spec",) + key not in _cache:
        f = lambda a: np.asarray(a, np.float64)                     # noqa: E731
        x1 = NC.cells_of(f(x))
        assert x1.shape[1] * x1.shape[2] <= 1100                    # the N x N spec stays small: class_reference beyond
        _cache[("spec",) + key] = pfnl_spec.depth_to_space2(x1 + pfnl_spec.nonlocal_block(x1, *[f(a) for a in w], stabilise=True))
    return _cache[("spec",) + key]


def _run(kernel, x, w):
    got = ops.nonlocal_residual(dev(x), *w, precision=kernel).cpu().numpy()
    assert np.isfinite(got).all(), kernel
    return got.astype(np.float64)


def _folded(w):
    wg, bg, ww, bw = (np.asarray(a, np.float64) for a in w)
    C = bg.size
    return wg.reshape(C, C) @ ww.reshape(C, C), bg @ ww.reshape(C, C) + bw


# ---- a. 8-bit families at small shapes -------------------------------------------------------------------------------------------------

FAMILIES = ["full", "dark", "saturated", "zeros", "ones", "sub_milli"]
SHAPES = [(16, 24), (2, 130), (62, 70)]                             # N = 96: one tile (and a half); 65: a partial last half; 1085: key splits


def _family(fam, T, H, W):
    key = (fam, T, H, W)
    if key not in _cache:
        rng = np.random.default_rng(sum(map(ord, fam)) + 1000 * T + 10 * H + W)
        shape = (1, T, H, W, 3)
        _cache[key] = NC.sub_milli(rng, shape) if fam == "sub_milli" else NC.PRESETS[fam](rng, shape)
    return _cache[key]


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("T", [3, 7])
@pytest.mark.parametrize("kernel", KERNELS)
def test_levels8_families(kernel, T, H, W):
    C = 12 * T
    w = _weights(T, C)
    Wf, bf = _folded(w)
    grid0 = np.zeros((1, H // 2, W // 2), np.int64)
    closed = {"zeros": NC.class_expand(bf[None, :], grid0),                           # b', the folded bias
              "ones": NC.class_expand((1.0 + Wf.sum(axis=0) + bf)[None, :], grid0)}   # 1 + W'^T 1 + b'
    worst = {}
    for fam in FAMILIES:
        x = _family(fam, T, H, W)
        got = _run(kernel, x, w)
        ref = _spec((fam, T, H, W), x, w)
        assert got.shape == ref.shape
        worst[fam] = float(np.abs(got - ref).max())
        if fam in closed:
            assert np.abs(closed[fam] - ref).max() < 1e-12
            worst[fam] = max(worst[fam], float(np.abs(got - closed[fam]).max()))
    print("levels8 %-7s T=%d %dx%d (ks %d):" % (kernel, T, H, W, NC.key_splits(1, H * W // 4)), "  ".join("%s %.2e" % kv for kv in worst.items()))
    for fam, e in worst.items():
        assert e < TOL[kernel], (kernel, fam, T, H, W, e)


@pytest.mark.parametrize("nltype", [1, 2])
@pytest.mark.parametrize("T,H,W", [(7, 16, 24), (3, 62, 70)])
def test_sub_milli_through_nonlocal_block(T, H, W, nltype):
    """Values under 0.001 through the general block with pooled keys (nl_pool_kernel, sub_sample = 2) as PFNL's Gaussian and as the
    dot product (nl_qproj_kernel with the per-query constant, relu / rowsum) against the fp64 spec."""
    C = 12 * T
    rng = np.random.default_rng(100 * T + nltype)
    x = _family("sub_milli", T, H, W)
    mk = lambda sc: (rng.normal(size=(1, 1, C, C)) * sc).astype(np.float32)      # noqa: E731
    wg, ww, wt, wp = mk(0.1), mk(0.1), mk(0.15), mk(0.15)
    bg, bw, bt, bp = ((rng.normal(size=C) * s).astype(np.float32) for s in (0.05, 0.05, 0.3, 0.3))
    if float(bt.astype(np.float64) @ bp.astype(np.float64)) < 0:    # x ~ 0: every affinity is ~ bt . bp - keep it positive, or the
        bp = -bp                                                    # relu leaves 0 / 0 for every query (NaN in the reference too)
    th, ph = ((wt, bt), (wp, bp)) if nltype == 2 else (None, None)
    got = ops.nonlocal_block(dev(x), wg, bg, ww, bw, theta=th, phi=ph, nltype=nltype, sub_sample=2).cpu().numpy()
    f = lambda a: a.astype(np.float64)                                           # noqa: E731
    x1 = NC.cells_of(f(x))
    z = pfnl_spec.nonlocal_block(x1, f(wg), f(bg), f(ww), f(bw), theta=None if th is None else (f(wt), f(bt)),
                                 phi=None if ph is None else (f(wp), f(bp)), nltype=nltype, sub_sample=2, stabilise=True)
    ref = pfnl_spec.depth_to_space2(x1 + z)
    assert np.isfinite(ref).all() and np.isfinite(got).all()
    err = float(np.abs(got - ref).max())
    print("sub_milli nonlocal_block nltype %d sub 2 T=%d %dx%d: %.2e" % (nltype, T, H, W, err))
    assert err < TOL["fp32"], err


# ---- b. identity projection, one dominant key ------------------------------------------------------------------------------------------

def _positions(N):
    last_tile = 64 * ((N - 1) // 64)
    return sorted({0, N - 1, last_tile} | ({63} if N > 64 else set()))


@pytest.mark.parametrize("B", [1, 32])
@pytest.mark.parametrize("N", [33, 65, 97, 129, 193])
@pytest.mark.parametrize("kernel", KERNELS)
def test_dominant_key_returns_its_value(kernel, N, B):
    """wg = ww = I, no biases: out - x is the attention mean.  One bright cell (levels 200..255) among dark ones (0..3): its own query
    has its top logit >= 40 above every other, the fp64 mean IS the cell to 1e-17, and the kernel must return it to the precision of
    its value operand: 2^-22 |v| (fp32, split16) or 2^-11 |v| (f16), plus the rounding of the residual add.  Every other query against
    its fp64 mean at the flat tolerance.  Positions: first key, last key of a full tile, last real key (N - 1: next to the rows masked
    through data), first key of the last tile.  B = 1: one call per position, every 64-key tile a key split of its own (nl_key_splits
    gives a handful of workgroups one tile each), so the dominant key lives in ONE part of the merge; B = 32: one call, clip b with
    the key at position b modulo the number of positions, unsplit - the whole chain in one workgroup."""
    T, C = 7, 84
    w = _identity(C)
    rel = 2.0 ** -11 if kernel == "f16" else 2.0 ** -22
    ks = (NC.key_splits if kernel == "fp32" else NC.key_splits_f16)(B, N)
    assert ks == (-(-N // 64) if B == 1 else 1)
    pos_all = _positions(N)
    worst, worst_rest = 0.0, 0.0
    for call in ([[p] for p in pos_all] if B == 1 else [[pos_all[b % len(pos_all)] for b in range(B)]]):
        rng = np.random.default_rng(1000 * N + call[0] + B)
        cells = NC.dark8(rng, (len(call), N, C))
        for b, pos in enumerate(call):
            cells[b, pos] = NC.levels8(rng, C, 200, 255)
        x = NC.clip_of(cells[:, None])                               # a 1 x N grid of cells per clip
        got = pfnl_spec.space_to_depth2(_run(kernel, x, w))[:, 0]    # [B, N, C]: out in the cells' layout
        for b, pos in enumerate(call):
            v = cells[b].astype(np.float64)
            f = v @ v.T
            assert f[pos, pos] - np.delete(f[pos], pos).max() >= 40.0
            p = np.exp(f - f.max(axis=1, keepdims=True))
            mean = (p / p.sum(axis=1, keepdims=True)) @ v
            assert np.abs(mean[pos] - v[pos]).max() <= 1e-17 * v[pos].max()
            d = got[b] - v                                           # out - x (exact in fp64)
            bound = rel * v[pos] + 2.0 ** -24 * v[pos]               # (the query is the key: x = v_key)
            worst = max(worst, worst_ratio(d[pos], v[pos], bound))
            worst_rest = max(worst_rest, float(np.abs(np.delete(d - mean, pos, axis=0)).max()))
    print("dominant key %-7s N=%3d B=%2d (ks %d) positions %s: worst |out - x - v| / bound %.3f; other queries %.2e"
          % (kernel, N, B, ks, pos_all, worst, worst_rest))
    assert worst <= 1.0, (kernel, N, worst)
    assert worst_rest < TOL[kernel], (kernel, N, worst_rest)


# ---- c. orderings of the running maximum, unequal key splits ---------------------------------------------------------------------------

def _ramp_cells(C):
    """32 brightness levels (7, 15, .. 255) under a fixed per-channel tint in [1/2, 1], as 8-bit levels."""
    tint = 0.5 + 0.5 * np.random.default_rng(5).random(C)
    return NC.dequant8(np.rint(np.arange(7, 256, 8)[:, None] * tint[None, :]).astype(np.uint8))


@pytest.mark.parametrize("order", ["ascending", "descending"])
@pytest.mark.parametrize("N,B", [(193, 16), (321, 16), (193, 1), (321, 1), (1024, 1)])
@pytest.mark.parametrize("kernel", KERNELS)
def test_ramps(kernel, N, B, order):
    """A maximum that rises at every 32-key half (alpha != 1 in every half-body) / that sits in the first half (every later probability a
    binary16 subnormal or zero).  N = 193 and 321 at B = 16 run unsplit (nl_key_splits keeps >= 4 tiles per split once 32 workgroups
    exist): 4 and 6 tiles turn the ring of 3 / 5 LDS slots more than once; at B = 1 every tile is a key split of its own - 4 / 6 parts
    with rising maxima to merge; N = 1024 at B = 1 merges 8 key splits of two tiles.  (The clips of a batch are equal: one reference.)"""
    T, C = 3, 36
    cells = _ramp_cells(C)
    ks = (NC.key_splits if kernel == "fp32" else NC.key_splits_f16)(B, N)
    assert ks == {(193, 16): 1, (321, 16): 1, (193, 1): 4, (321, 1): 6, (1024, 1): 8}[N, B]
    H, W = (2, 2 * N) if N != 1024 else (64, 64)
    grid = getattr(NC, order)(cells, N).reshape(1, H // 2, W // 2)
    x = NC.palette_clip(cells, grid)
    w = _weights(3, C)
    ref = _spec((order, N), x, w)
    got = _run(kernel, np.repeat(x, B, axis=0), w)
    err = float(np.abs(got - ref).max())
    print("ramp %-10s %-7s N=%4d B=%2d (ks %d): %.2e" % (order, kernel, N, B, ks, err))
    assert err < TOL[kernel], err


@pytest.mark.parametrize("confined", ["saturated", "zeros"])
@pytest.mark.parametrize("sp", [0, 7])
@pytest.mark.parametrize("kernel", KERNELS)
def test_block_in_one_key_split(kernel, sp, confined):
    """64 x 64 at B = 1: 8 key splits of 128 keys.  A saturated block (levels 252..255, base-2 logit ~ 121) confined to split sp with every
    other cell exactly zero (m_p = 0 next to m_p ~ 121 in nl_merge_kernel), and the reverse: the zero cells confined to one split."""
    T, C, N = 7, 84, 1024
    assert NC.key_splits(1, N) == 8 and NC.key_splits_f16(1, N) == 8
    cells = np.stack([np.zeros(C, np.float32), NC.levels8(np.random.default_rng(sp), C, 252, 255)])
    entry, other = (1, 0) if confined == "saturated" else (0, 1)
    flat = NC.block_in_split(sp, 8, N, entry=entry, other=other)
    grid = flat.reshape(1, 32, 32)
    x = NC.palette_clip(cells, grid)
    w = _weights(7, C)
    ref = NC.class_expand(NC.class_reference(cells, np.bincount(flat, minlength=2), *w), grid)
    err = float(np.abs(_run(kernel, x, w) - ref).max())
    print("block in split %d of 8, %-9s confined, %-7s: %.2e" % (sp, confined, kernel, err))
    assert err < TOL[kernel], err


# ---- d. long chains --------------------------------------------------------------------------------------------------------------------

LEVELS = (100, 235, 77)
LONG_FAMILIES = ["flat100", "flat235", "flat77", "two-tone halves", "two-tone stripes"]


def _long_grid(fam, h, w):
    """Flat index grid into the palette flat_cells(LEVELS) of one clip of a long-chain family."""
    N = h * w
    if fam.startswith("flat"):
        return np.full(N, LEVELS.index(int(fam[4:])), np.int64)
    if fam == "two-tone halves":                                    # 100 on the first half of the keys, 235 on the rest
        return (np.arange(N) >= N // 2).astype(np.int64)
    return np.where(np.arange(N) // 8 % 2 == 0, 2, 1)               # stripes of 8 keys: 77 | 235


@pytest.mark.parametrize("B,H,W", [(16, 128, 128), (5, 256, 256), (1, 256, 256)])
@pytest.mark.parametrize("kernel", KERNELS)
def test_long_chains_on_flat_and_two_tone_frames(kernel, B, H, W):
    """(B = 16, 128 x 128) and (B = 5, 256 x 256) run unsplit - nl_key_splits: ceil(512 / (ceil(N / 128) B)) = 1 - as ONE chain of 4096 /
    16384 keys per query; (B = 1, 256 x 256) as 4 merged chains of 4096.  Clip b of a batch holds family b mod 5 (B = 1: one call per
    family).  Pass condition: nl_content.attention_bound, element-wise against nl_content.class_reference.  The error against the
    suite's flat tolerance (2e-5 / 2e-3) is printed as a measurement.  Measured on the MI355X (worst bound ratio; |err| at 4096 | 16384 keys
    per chain): fp32 0.17, 8.5e-5 | 2.8e-4 - beyond 2e-5 from 4096 keys; split16 0.25, 1.4e-5 | 8.5e-5 - beyond 2e-5 at 16384; f16 0.20,
    5.3e-4 | 5.8e-4 - inside 2e-3.  The merge of 4 chains of 4096 is as good as one chain of 4096."""
    T, C = 3, 36
    h, w_ = H // 2, W // 2
    N = h * w_
    ks = (NC.key_splits if kernel == "fp32" else NC.key_splits_f16)(B, N)
    assert ks == (4 if B == 1 else 1)
    chain = NC.longest_chain(N, ks)
    cells = NC.flat_cells(LEVELS, C)
    w = _weights(11, C)
    batches = [[f] for f in LONG_FAMILIES] if B == 1 else [[LONG_FAMILIES[b % 5] for b in range(B)]]
    for fams in batches:
        grids = np.stack([_long_grid(f, h, w_) for f in fams]).reshape(len(fams), h, w_)
        got = _run(kernel, NC.palette_clip(cells, grids), w)
        for fam in dict.fromkeys(fams):
            b = fams.index(fam)
            counts = np.bincount(grids[b].ravel(), minlength=len(cells))
            if ("long", fam, N, kernel, ks) not in _cache:
                _cache["long", fam, N, kernel, ks] = (NC.class_reference(cells, counts, *w),
                                                      NC.attention_bound(kernel, cells, counts, *w, chain_keys=chain, ks=ks))
            rows, brows = _cache["long", fam, N, kernel, ks]
            sel = [i for i, f in enumerate(fams) if f == fam]
            ref = NC.class_expand(rows, grids[sel])
            bound = NC.class_expand(brows, grids[sel])
            err = float(np.abs(got[sel] - ref).max())
            r = worst_ratio(got[sel], ref, bound)
            print("long chain %-7s B=%2d %dx%d chain %5d x %d  %-16s bound ratio %.3f   |err| %.2e = %.2f of the flat tolerance %.0e"
                  % (kernel, B, H, W, chain, ks, fam, r, err, err / TOL[kernel], TOL[kernel]))
            assert r <= 1.0, (kernel, B, H, W, fam, r, err)


# ---- e. flat frames at non-dyadic levels, 16 x 16 ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("level", [0.3, 100 / 255.])
@pytest.mark.parametrize("kernel", KERNELS)
def test_nonlocal_constant_non_dyadic(kernel, level):
    """The companion of test_nonlocal_constant_and_peaked_inputs (constant 0.25: exactly representable sums) at 0.3 and 100 / 255."""
    T, H, W = 7, 16, 16
    C = 12 * T
    w = _weights(0, C)
    x = np.full((1, T, H, W, 3), level, np.float32)
    Wf, bf = _folded(w)
    lv = np.float64(np.float32(level))
    ref = NC.class_expand((lv + lv * Wf.sum(axis=0) + bf)[None, :], np.zeros((1, H // 2, W // 2), np.int64))
    err = float(np.abs(_run(kernel, x, w) - ref).max())
    print("constant %.4f %-7s: %.2e" % (level, kernel, err))
    assert err < (1e-5 if kernel != "f16" else TOL["f16"]), err


def test_stress_nl_levels8_short():
    """A short run of tools/stress_nl.py on 8-bit content: random geometries, random level ranges, against the fp64 spec."""
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    import stress_nl
    n, worst = stress_nl.run(seed=5, seconds=6.0, max_iters=30, content="levels8")
    print("stress_nl levels8: %d geometries, worst %s" % (n, worst))
    assert n >= 10 and worst["split16"] < TOL["split16"] and worst["f16"] < TOL["f16"], (n, worst)
