"""Host checks of tests/nl_content.py: the closed-form reference against the fp64 spec, the generators, the key-split arithmetic, the
error bound against a float32 emulation of the accumulation chains, and that two wrong kernels (no alpha rescale; a merge with equal
weights) would be caught on the families test_gpu_nl_content.py runs."""
import numpy as np
import pytest

import nl_content as NC
from oracle import pfnl_spec


def _weights(rng, C):
    wg = (rng.normal(size=(1, 1, C, C)) / np.sqrt(C)).astype(np.float32)
    ww = (rng.normal(size=(1, 1, C, C)) / np.sqrt(C)).astype(np.float32)
    return wg, rng.normal(size=C).astype(np.float32) * 0.1, ww, rng.normal(size=C).astype(np.float32) * 0.1


def _spec(x, wg, bg, ww, bw):
    f = lambda a: np.asarray(a, np.float64)                         # noqa: E731
    x1 = NC.cells_of(f(x))
    z = pfnl_spec.nonlocal_block(x1, f(wg), f(bg), f(ww), f(bw), stabilise=True)
    return pfnl_spec.depth_to_space2(x1 + z)


@pytest.mark.parametrize("T", [3, 7])
@pytest.mark.parametrize("k", [1, 2, 5])
def test_class_reference_is_the_spec(T, k):
    rng = np.random.default_rng(10 * T + k)
    C = 12 * T
    cells = NC.levels8(rng, (k, C))
    if k > 1:
        cells[1] = 0.0                                              # an exactly-zero cell (letterbox black)
    wg, bg, ww, bw = _weights(rng, C)
    for B, h, w in ((1, 1, 1), (2, 3, 5), (1, 16, 16)):
        grid = rng.integers(0, k, size=(B, h, w))
        x = NC.palette_clip(cells, grid)
        assert x.shape == (B, T, 2 * h, 2 * w, 3) and x.dtype == np.float32
        assert np.array_equal(NC.cells_of(x), cells[grid])          # the channel order of space_to_depth2
        ref = _spec(x, wg, bg, ww, bw)
        got = np.concatenate([NC.class_expand(NC.class_reference(cells, np.bincount(grid[b].ravel(), minlength=k), wg, bg, ww, bw),
                                              grid[b:b + 1]) for b in range(B)])
        assert got.shape == ref.shape
        assert np.abs(got - ref).max() <= 1e-12, np.abs(got - ref).max()


def test_generators_stay_in_range_and_levels_are_the_dequantised_bytes():
    rng = np.random.default_rng(0)
    shape = (2, 3, 8, 12, 3)
    table = (np.arange(256, dtype=np.uint8) / 255.).astype(np.float32)
    for name, gen in NC.PRESETS.items():
        x = gen(rng, shape)
        assert x.dtype == np.float32 and x.shape == shape and x.min() >= 0.0 and x.max() <= 1.0, name
        u = np.rint(x.astype(np.float64) * 255).astype(np.uint8)
        assert np.array_equal(x.view(np.uint32), table[u].view(np.uint32)), name      # bit-identical to u8 / 255.
    assert np.array_equal(NC.levels8(np.random.default_rng(3), shape, 7, 9).view(np.uint32),
                          (np.random.default_rng(3).integers(7, 10, size=shape).astype(np.uint8) / 255.).astype(np.float32).view(np.uint32))
    d = NC.PRESETS["dark"](rng, (4, 3, 16, 16, 3))
    assert d.max() <= np.float32(3 / 255.) and (d == 0).mean() >= 1.0 / 3.0
    s = NC.PRESETS["saturated"](rng, shape)
    assert s.min() >= np.float32(252 / 255.) and s.max() == 1.0
    assert not NC.PRESETS["zeros"](rng, shape).any() and (NC.PRESETS["ones"](rng, shape) == 1.0).all()
    m = NC.sub_milli(rng, shape)
    assert m.dtype == np.float32 and m.min() > 0.0 and m.max() < 0.001
    cells = NC.flat_cells([0, 100, 255], 36)
    x = NC.palette_clip(cells, rng.integers(0, 3, size=(1, 4, 6)))
    assert x.min() == 0.0 and x.max() == 1.0


def test_orderings():
    cells = NC.flat_cells(np.arange(7, 256, 8), 36)                 # 32 brightness levels
    perm = np.random.default_rng(1).permutation(32)
    cells = cells[perm]
    lg = NC.self_logit(cells)
    for N in (33, 193, 321, 1024):
        up, down = NC.ascending(cells, N), NC.descending(cells, N)
        assert np.all(np.diff(lg[up]) >= 0) and np.all(np.diff(lg[down]) <= 0)
        assert len(set(up)) == 32 and len(set(down)) == 32 and up[0] == down[-1] and up[-1] == down[0]
        assert np.bincount(up, minlength=32).min() >= N // 32
    g = NC.dominant_at(64, 129)
    assert g.sum() == 1 and g[64] == 1 and g.shape == (129,)


@pytest.mark.parametrize("N,ks", [(1024, 8), (16384, 4), (2170, 3), (193, 3), (64, 1), (321, 5), (100, 2)])
def test_block_in_split_is_the_kernels_tile_range(N, ks):
    ntiles = -(-N // 64)
    owner = np.full(N, -1)
    for sp in range(ks):                                            # literally: for (kt = kt0; kt < kt1; ++kt) keys kt * 64 .. + 63, below N
        for kt in range(ntiles * sp // ks, ntiles * (sp + 1) // ks):
            for key in range(kt * 64, min(kt * 64 + 64, N)):
                assert owner[key] == -1
                owner[key] = sp
    assert (owner >= 0).all()                                       # the splits tile the keys
    for sp in range(ks):
        assert np.array_equal(NC.block_in_split(sp, ks, N) == 1, owner == sp)
        assert np.array_equal(NC.block_in_split(sp, ks, N, entry=0, other=1) == 0, owner == sp)
    assert NC.longest_chain(N, ks) == np.bincount(owner).max()


def test_key_split_counts_of_the_geometries_used():
    """The geometries test_gpu_nl_content.py relies on (nl_key_splits of nonlocal.hip, the f16 kernels' own choice below it)."""
    assert NC.key_splits(16, 4096) == 1 and NC.key_splits(4, 16384) == 1
    assert NC.key_splits(1, 16384) == 4 and NC.key_splits_f16(1, 16384) == 4
    assert NC.key_splits(1, 1024) == 8 and NC.key_splits_f16(1, 1024) == 8
    assert NC.key_splits(1, 31 * 35) > 1                            # 62 x 70: the key-split path
    assert NC.key_splits(1, 64) == 1 and NC.key_splits(1, 96) == 2          # (a handful of workgroups: one tile each)


LEVELS = (100, 235, 77)
CHAINS = (4096, 16384)                                              # (B = 16, 128 x 128) and (B = 4, 256 x 256); B = 1, 256 x 256: 4 x 4096


def _families(C=36):
    """(name, cells [k, C], flat index grid builder) of the long-chain tests: flat frames and two-tone frames."""
    fam = [("flat%d" % lv, NC.flat_cells([lv], C), lambda N: np.zeros(N, np.int64)) for lv in LEVELS]
    two = NC.flat_cells([LEVELS[0], LEVELS[1]], C)
    fam.append(("two-tone halves", two, lambda N: (np.arange(N) >= N // 2).astype(np.int64)))
    fam.append(("two-tone stripes", NC.flat_cells([LEVELS[2], LEVELS[1]], C), lambda N: (np.arange(N) // 8 % 2).astype(np.int64)))
    return fam


def test_float32_chain_stays_inside_the_bound_and_breaks_the_sqrt_model():
    """The arithmetic the bound describes, emulated: one float32 accumulator over the keys in order (1, 2 or 16 products per update),
    on the flat and two-tone families at the chain lengths the GPU tests run.  It must meet nl_content.mean_bound - the reference
    arithmetic alone meets the bound - and on flat content it must exceed 2^-24 sqrt(n) A, the statistical model of numerics.alpha:
    the family is not already covered by it."""
    C = 36
    worst, over_sqrt = {}, []
    for name, cells, grid_of in _families(C):
        for n in CHAINS:
            grid = grid_of(n)
            counts = np.bincount(grid, minlength=len(cells))
            P, mean, A, D, L = NC.class_stats(cells, counts)
            absum = np.abs(cells.astype(np.float64)).sum(axis=1)
            for a in range(len(cells)):
                f = cells[a].astype(np.float64) @ cells.astype(np.float64).T
                w = np.exp(f - f.max())[grid]
                for per_step, kernel in ((1, "fp32"), (2, "fp32"), (16, "split16"), (16, "f16")):
                    got = NC.chain_mean_f32(cells[grid][:, :1], w, per_step)          # (every channel of a cell is equal: one is enough)
                    err = np.abs(got - mean[a, :1])
                    bound = NC.mean_bound(kernel, A[a, :1], D[a, :1], L[a], absum[a] + absum.max(), C, n, n)
                    r = float((err / bound).max())
                    key = (name.split()[0].rstrip("0123456789"), kernel, per_step)
                    worst[key] = max(worst.get(key, 0.0), r)
                    assert r <= 1.0, (name, n, a, per_step, kernel, err, bound)
                    if name.startswith("flat") and per_step <= 2:
                        over_sqrt.append((name, n, per_step, float(err.max() / (NC.U32 * np.sqrt(n) * A[a, 0]))))
    for key, r in sorted(worst.items()):
        print("emulated chain / bound  %-9s %-8s %2d products per update: %.3f" % (key + (r,)))
    print("flat content, error / (2^-24 sqrt(n) A):", ["%s n=%d /%d: %.1f" % o for o in over_sqrt])
    assert max(o[3] for o in over_sqrt) > 1.0
    assert sum(o[3] > 1.0 for o in over_sqrt) >= len(over_sqrt) // 2           # ... and not by accident on one level


def test_a_dyadic_level_cannot_show_the_drift():
    """0.25 (the constant of test_nonlocal_constant_and_peaked_inputs) accumulates exactly: the reason for the non-dyadic levels."""
    v = np.full((16384, 1), 0.25, np.float32)
    assert NC.chain_mean_f32(v, np.ones(16384), 1)[0] == 0.25
    assert NC.chain_mean_f32(NC.flat_cells([100], 1).repeat(16384, axis=0), np.ones(16384), 1)[0] != np.float64(np.float32(100 / 255.))


def _true_mean(X):
    X = X.astype(np.float64)
    f = X @ X.T
    p = np.exp(f - f.max(axis=1, keepdims=True))
    return (p / p.sum(axis=1, keepdims=True)) @ X


@pytest.mark.parametrize("N", [193, 321])
def test_a_kernel_without_the_alpha_rescale_fails_the_ascending_family(N):
    cells = NC.flat_cells(np.arange(7, 256, 8), 36)
    X = cells[NC.ascending(cells, N)]
    ref = _true_mean(X)
    good = np.abs(NC.streaming_attention(X) - ref).max()
    bad = np.abs(NC.streaming_attention(X, drop_alpha=True) - ref).max()
    print("ascending N=%d: streaming softmax %.2e, without the rescale %.2e (tolerance %.0e)" % (N, good, bad, NC.FLAT_TOL["fp32"]))
    assert good < NC.FLAT_TOL["fp32"] < NC.FLAT_TOL["f16"] < bad
    X = cells[NC.descending(cells, N)]                               # (the maximum comes first: nothing to rescale, nothing caught)
    assert np.abs(NC.streaming_attention(X, drop_alpha=True) - _true_mean(X)).max() < NC.FLAT_TOL["fp32"]


@pytest.mark.parametrize("sp", [0, 7])
def test_a_merge_with_equal_weights_fails_the_block_in_split_family(sp):
    N, ks = 1024, 8
    rng = np.random.default_rng(sp)
    cells = np.stack([np.zeros(36, np.float32), NC.levels8(rng, 36, 252, 255)])
    for entry, other in ((1, 0), (0, 1)):                           # a saturated block in one split; the zero cells in one split
        X = cells[NC.block_in_split(sp, ks, N, entry=entry, other=other)]
        ref = _true_mean(X)
        good = np.abs(NC.streaming_attention(X, ks=ks) - ref).max()
        bad = np.abs(NC.streaming_attention(X, ks=ks, equal_merge=True) - ref).max()
        print("block_in_split sp=%d entry=%d: merged %.2e, equal weights %.2e" % (sp, entry, good, bad))
        assert good < NC.FLAT_TOL["fp32"] < NC.FLAT_TOL["f16"] < bad
