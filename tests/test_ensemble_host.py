"""The self-ensemble's device-free side: the rule (pfnl_amd/ensemble.py: members, transform, inverse, combine) and the argument checks of
the C-ABI and of open_stream that need no device (include/pfnl_hip.h SELF-ENSEMBLE)."""
import ctypes as C
import itertools

import numpy as np
import pytest

from pfnl_amd import _capi, ensemble


def _distinct(shape):
    return np.arange(int(np.prod(shape)), dtype=np.float32).reshape(shape)


def test_members_and_refusals():
    assert [list(ensemble.members(n)) for n in (1, 2, 4, 8)] == [[0], [0, 1], [0, 1, 2, 3], list(range(8))]
    for n in (0, 3, 5, 6, 7, 16, -1, 2.0, "2", None, True):
        with pytest.raises(ValueError):
            ensemble.members(n)
    x = _distinct((2, 6, 10, 3))
    for k in (-1, 8, 1.0, None):
        with pytest.raises(ValueError):
            ensemble.transform(x, k)
        with pytest.raises(ValueError):
            ensemble.inverse(x, k)
    with pytest.raises(ValueError):
        ensemble.combine(lambda a: a, x, 3)


def test_inverse_undoes_transform_and_the_members_differ():
    x = _distinct((2, 6, 10, 3))
    images = []
    for k in range(8):
        g = ensemble.transform(x, k)
        assert g.flags["C_CONTIGUOUS"] and g.dtype == x.dtype
        assert g.shape == ((2, 10, 6, 3) if k >= 4 else (2, 6, 10, 3))          # shapes swap for the transposing members
        assert np.array_equal(ensemble.inverse(g, k), x)
        assert np.array_equal(ensemble.transform(ensemble.inverse(g, k), k), g)
        assert np.array_equal(np.sort(g.ravel()), x.ravel())                     # a permutation of the entries
        images.append(g)
    for a, b in itertools.combinations(range(8), 2):
        assert images[a].shape != images[b].shape or not np.array_equal(images[a], images[b]), (a, b)


def test_the_rule_element_by_element():
    # bit 0 mirrors W, bit 1 mirrors H, bit 2 transposes and is applied last - on single entries, independent of numpy's slicing
    x = _distinct((4, 6, 3))
    H, W = 4, 6
    for k in range(8):
        g = ensemble.transform(x, k)
        for i in range(H):
            for j in range(W):
                si, sj = (H - 1 - i if k & 2 else i), (W - 1 - j if k & 1 else j)   # a = mirrored x: a[i][j] = x[si][sj]
                got = g[j, i] if k & 4 else g[i, j]
                assert np.array_equal(got, x[si, sj]), (k, i, j)


def test_combine_returns_a_commuting_forward_exactly():
    # 4 x nearest-neighbour repeat commutes with every member: each member's result, transformed back, is the plain result
    up = lambda a: np.repeat(np.repeat(a, 4, axis=-3), 4, axis=-2)               # noqa: E731
    # The members' results are then n equal values v per element, and the rule sums them one at a time in float32.  Pixel values
    # u / 256 with u < 2^16 keep every partial sum 2v .. 8v exact (19 significant bits at the most), so the mean is v itself for every n.
    rng = np.random.default_rng(5)
    x = rng.integers(0, 1 << 16, (2, 6, 10, 3)).astype(np.float32) / np.float32(256)
    want = up(x)
    assert want.shape == (2, 24, 40, 3)
    for n in (1, 2, 4, 8):
        got = ensemble.combine(up, x, n)
        assert got.dtype == np.float32 and np.array_equal(got, want), n
    # on full 24-bit mantissas 2v is exact, 3v rounds and v + fl(3v) rounds back onto 4v: n = 2 and 4 stay exact (5v .. 7v need not)
    xf = rng.random((2, 6, 10, 3), dtype=np.float32)
    for n in (2, 4):
        assert np.array_equal(ensemble.combine(up, xf, n), up(xf)), n


def test_combine_of_a_forward_that_does_not_commute_is_the_fp64_mean():
    # The bound is 1 ulp of float32 at the result.  The rule rounds once per member: on full 24-bit mantissas n - 1 roundings of running
    # sums up to n times the result add up to (n - 1) / 2 ulp of the result at the worst - above 1 ulp from n = 4 on.  So the inputs sit
    # on a grid: x in multiples of 2^-12 below 1, a ramp in sixteenths below 1.  Every member's result is a multiple of 2^-12 below 2,
    # every partial sum a multiple of 2^-12 below 16 - 16 significant bits, exact in float32 - and what remains to differ is the rule
    # itself: which entry of which member's result lands where.  On full mantissas the bound holds for n = 2 (one rounding: half an
    # ulp of the sum, which is half an ulp of the mean), checked as well.
    rng = np.random.default_rng(6)
    grid = rng.integers(0, 1 << 12, (2, 6, 10, 3)).astype(np.float32) / np.float32(1 << 12)
    full = rng.random((2, 6, 10, 3), dtype=np.float32)

    def ramp(a):                                                                 # adds a ramp along the array's own W axis
        return a + (np.arange(a.shape[-2], dtype=np.float32) / np.float32(16))[:, None]

    for n, x in ((2, grid), (4, grid), (8, grid), (2, full)):
        got = ensemble.combine(ramp, x, n)
        # by hand, in float64, from the member results in float32 (what a forward returns)
        mean = np.zeros(x.shape, np.float64)
        for k in range(n):
            a = x
            if k & 1:
                a = a[..., :, ::-1, :]
            if k & 2:
                a = a[..., ::-1, :, :]
            if k & 4:
                a = np.swapaxes(a, -3, -2)
            y = ramp(np.ascontiguousarray(a)).astype(np.float32)
            if k & 4:
                y = np.swapaxes(y, -3, -2)
            if k & 2:
                y = y[..., ::-1, :, :]
            if k & 1:
                y = y[..., :, ::-1, :]
            mean += y.astype(np.float64)
        mean /= n
        assert got.dtype == np.float32
        assert np.all(np.abs(got.astype(np.float64) - mean) <= np.spacing(np.abs(mean).astype(np.float32))), n
        assert not np.array_equal(got, ramp(x))                                  # the members do differ


def test_capi_refuses_without_a_device():
    lib = _capi.load_library()
    assert lib.pfnl_version() == 4
    dummy = C.c_void_p(16)                                                       # never dereferenced: the calls return first
    for n in (3, 16, 0, -2):
        assert lib.pfnl_forward_ensemble(dummy, dummy, 1, dummy, 1, 1, 16, 24, n, None) == -1
        assert b"ensemble" in lib.pfnl_last_error()
    assert lib.pfnl_forward_ensemble(None, dummy, 1, dummy, 1, 1, 16, 24, 8, None) == -1 and b"NULL" in lib.pfnl_last_error()
    assert lib.pfnl_forward_ensemble(None, dummy, 1, dummy, 1, 1, 16, 24, 1, None) == -1 and b"NULL" in lib.pfnl_last_error()
    one = C.c_float(1.0)
    for fn in (lib.pfnl_op_dihedral, lib.pfnl_op_dihedral_accum):
        assert fn(None, dummy, 1, 6, 10, 0, one, None) == -1 and b"NULL" in lib.pfnl_last_error()
        assert fn(dummy, None, 1, 6, 10, 0, one, None) == -1 and b"NULL" in lib.pfnl_last_error()
        assert fn(dummy, dummy, 1, 6, 10, 8, one, None) == -1 and b"0 .. 7" in lib.pfnl_last_error()
        assert fn(dummy, dummy, 1, 6, 10, -1, one, None) == -1 and b"0 .. 7" in lib.pfnl_last_error()
        for n_img, H, W in [(0, 6, 10), (1, 0, 10), (1, 6, -4)]:
            assert fn(dummy, dummy, n_img, H, W, 1, one, None) == -1 and b"positive" in lib.pfnl_last_error()
    assert lib.pfnl_stream_ensemble(None, 8) == -1 and b"NULL" in lib.pfnl_last_error()
    assert lib.pfnl_stream_ensemble(dummy, 3) == -1 and b"ensemble" in lib.pfnl_last_error()


def test_open_stream_host_check_refuses_a_bad_ensemble():
    import inspect

    from pfnl_amd.engine import PFNLEngine, ensemble_members
    from pfnl_amd.model import PFNL
    from pfnl_amd.stream import VideoStream, ensemble_argument
    assert [ensemble_argument(n) for n in (1, 2, 4, 8)] == [1, 2, 4, 8] and ensemble_argument() == 1
    for bad in (3, 16, 0, "8", None, 2.5):
        with pytest.raises(ValueError):
            ensemble_argument(bad)
        with pytest.raises(ValueError):
            ensemble_members(bad)
    for f in (PFNLEngine.open_stream, PFNL.open_stream, VideoStream.__init__):   # a new LAST keyword, off by default
        name, p = list(inspect.signature(f).parameters.items())[-1]
        assert (name, p.default) == ("ensemble", 1), f
    assert inspect.signature(PFNLEngine.forward).parameters["ensemble"].default is None
    assert inspect.signature(PFNLEngine.forward_device).parameters["ensemble"].default == 1
    assert PFNL().self_ensemble == 1

    class Unready:                                                               # the check comes before anything touches the engine
        pass
    with pytest.raises(ValueError, match="ensemble"):
        VideoStream(Unready(), 16, 24, 1, ensemble=3)
