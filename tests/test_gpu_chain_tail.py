"""The tail of the conv2_i chain launches (conv3x3_sf_chain16_kernel, conv3x3_sf_chain_kernel; reference model/pfnl.py:69-71): the code
behind the tile loop is the only place where a workgroup's LAST tile gets its residual - all 2 rows x 4 quarters are requested in one
block of loads in front of the first store.  Pinned exactly: v + 0.0f is exact, so the launch with a residual R must equal
float32(launch with residual 0 + R) bit for bit - a swapped quarter, row, pixel or channel among the hoisted loads fails on the first
element.  Shapes are the smallest at which the tail can go wrong (see CASES); everything goes through ops.conv2_chain_ex."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from numerics import split_host  # noqa: E402
from pfnl_amd import ops  # noqa: E402


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _grid():
    """The grid of the persistent launches on this device (persistent_grid: the CU count rounded down to whole XCDs, at least 8)."""
    return max(8, torch.cuda.get_device_properties(0).multi_processor_count // 8 * 8)


def _geometry(name):
    """(clips, T, H, W, split) of a case; tiles are 8 rows x 32 columns, a chain = the T + 1 tiles of one (clip, spatial tile)."""
    G = _grid()
    if name == "two-tiles":                # one chain of two tiles: the only frame tile is the last tile
        return 1, 1, 8, 32, (0, 0, 0)
    if name == "ragged":                   # ragged bottom rows and right columns: rows of the last tile outside the image (empty resources)
        return 1, 3, 13, 45, (0, 0, 0)
    if name == "fewer-chains":             # fewer chains than workgroups: every workgroup's first chain is its last
        return 2, 7, 20, 70, (0, 0, 0)
    if name == "second-chain":             # a few more chains than workgroups: some run two chains, their last tile belongs to the second
        return 1, 1, 56, 32 * -(-(G + 3) // 7), (0, 0, 0)
    if name == "split":                    # 1.25 rounds of one-tile clips, T = 3: the plan's cut of 5 clips' partial round, scaled down -
        R = G // 4                         # R = G / 4 chains cut into s = min(T, G / R) = 3 parts of q = 1 frame (the SPLIT instantiations)
        return G + R, 3, 8, 32, (G, 3, 1)
    raise KeyError(name)


UNCUT = ["two-tiles", "ragged", "fewer-chains", "second-chain"]


@functools.lru_cache(maxsize=None)
def _inputs(name):
    clips, T, H, W, split = _geometry(name)
    rng = np.random.default_rng(sum(map(ord, name)))
    F = clips * T
    x = rng.standard_normal((F, H, W, 64), dtype=np.float32)
    base = rng.standard_normal((clips, H, W, 64), dtype=np.float32)
    R = rng.standard_normal((F, H, W, 64), dtype=np.float32)       # O(1), distinct per element for all a test can tell
    k2 = (rng.standard_normal((3, 3, 128, 64)) / 34.0).astype(np.float32)
    b = (rng.standard_normal(64) * 0.1).astype(np.float32)
    return T, split, x, base, R, k2, b, dev(x), dev(base), dev(R), torch.zeros((F, H, W, 64), dtype=torch.float32, device="cuda")


def _launch(name, mfma, act, with_resid):
    T, split, x, base, R, k2, b, xd, bd, rd, zd = _inputs(name)
    return ops.conv2_chain_ex(xd, k2, b, bd, rd if with_resid else zd, T, act=act, mfma=mfma, split=split).cpu().numpy()


_first = functools.lru_cache(maxsize=None)(_launch)                # the first launch of a (case, shape, act, residual): shared, never written


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _first.cache_clear()
    _inputs.cache_clear()


@pytest.mark.parametrize("act", [True, False])
@pytest.mark.parametrize("name,mfma", [(n, m) for n in UNCUT for m in (16, 32)] + [("split", 32)])
def test_residual_identity(name, mfma, act):
    """out(resid = R) == float32(out(resid = 0) + R), bit for bit, everywhere."""
    R = _inputs(name)[4]
    out0, outR = _first(name, mfma, act, False), _first(name, mfma, act, True)
    want = out0 + R                                                 # float32 + float32: the kernel's one v_add_f32
    bad = np.argwhere(outR.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (len(bad), bad[:4], outR[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("name", UNCUT + ["split"])
def test_repeats_and_mfma_shapes_agree(name):
    """Each launch repeats bit for bit; the 16x16x32 and the 32x32x16 form agree within summation order (test_chain_launch_mfma_shapes' bound)."""
    shapes = (32,) if name == "split" else (16, 32)
    for mfma in shapes:
        again = _launch(name, mfma, True, True)
        assert np.array_equal(again.view(np.uint32), _first(name, mfma, True, True).view(np.uint32)), mfma
    if len(shapes) == 2:
        a, c = _first(name, 16, True, True), _first(name, 32, True, True)
        d = np.abs(a - c).max()
        assert d < 2e-6 * max(1.0, np.abs(c).max()), d


def test_sfcopy_tail():
    """conv3x3_sf_chain_kernel<true, .>: the fp32 output equals the launch without the copy bit for bit, and the split-format copy is the
    split of that output (the host restatement of the split: numerics.split_host) - the ragged case, whose last tile has rows outside."""
    T, split, x, base, R, k2, b, xd, bd, rd, zd = _inputs("ragged")
    out, out_sf = ops.conv2_chain_sf0(xd, k2, b, bd, rd, T)
    out, out_sf = out.cpu().numpy(), out_sf.cpu().numpy()
    assert np.array_equal(out.view(np.uint32), _first("ragged", 32, True, True).view(np.uint32))
    want = split_host(out)
    bad = np.argwhere(out_sf != want)
    assert bad.size == 0, (len(bad), bad[:4], out_sf[tuple(bad[0])], want[tuple(bad[0])])
