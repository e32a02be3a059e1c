"""tests/history.py on the host (no GPU): the arena's check can fail - a single flipped bit in a gap, an output element left at its
fill - and accepts an untouched arena; the plan search, fed launch_plan.h's rule through tests/plan_driver.py, reaches every structure
tests/test_gpu_history.py lists, at 256 CUs and at another count."""
import numpy as np
import pytest

import history as Hy
from plan_driver import build, fields

torch = pytest.importorskip("torch")


def _arena(dtype="float32"):
    rng = np.random.default_rng(3)
    tdt = {"float32": torch.float32, "bfloat16": torch.bfloat16, "int16": torch.int16}[dtype]
    x = torch.from_numpy(rng.normal(size=(2, 9, 33, 64)).astype(np.float32)).to(tdt)
    b = torch.from_numpy(rng.normal(size=(1, 9, 33, 64)).astype(np.float32)).to(tdt)
    frame = 9 * 33 * 64 * Hy.ITEMSIZE[dtype]
    return Hy.Arena({"x": (tuple(x.shape), dtype, x), "base": (tuple(b.shape), dtype, b), "out": (tuple(x.shape), dtype, None)}, frame, device="cpu"), x, b


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "int16"])
def test_arena_layout_and_untouched_check(dtype):
    """Operands 256-byte aligned, contiguous, equal to their data; gaps of at least a frame in front, between and behind; an untouched
    arena whose output has been written passes; gaps hold the fill of the operand next to them."""
    a, x, b = _arena(dtype)
    frame = 9 * 33 * 64 * Hy.ITEMSIZE[dtype]
    assert torch.equal(a["x"], x) and torch.equal(a["base"], b)
    ends = [0] + [e for _, _, e, _, _ in a.spans]
    begins = [s for _, s, _, _, _ in a.spans] + [a.nbytes]
    for e, s in zip(ends, begins):
        assert s - e >= frame
    for name, s, e, _, _ in a.spans:
        assert (a.buf.data_ptr() + a.base + s) % 256 == 0 and a[name].is_contiguous() and a[name].data_ptr() == a.buf.data_ptr() + a.base + s
    if dtype != "int16":
        img = torch.from_numpy(a.image[:a.spans[0][1]].copy()).view(a["x"].dtype)
        assert bool(torch.isnan(img).all())                          # what a read in front of `x` meets
        assert bool(torch.isnan(a["out"]).all())
    else:
        assert bool((a["out"] == 0x7FFF).all())
    r = a.check()
    assert not r.ok and r.changed is None and r.unwritten == {"out": a["out"].numel()}    # nothing has written `out` yet
    a["out"].copy_(x)
    r = a.check()
    assert r.ok and r.changed_bytes == 0, str(r)
    a["x"].zero_()                                                   # an operand may change: only gaps and outputs are judged
    assert a.check().ok


@pytest.mark.parametrize("where", ["front", "after_x", "before_out", "tail"])
def test_arena_reports_a_single_flipped_bit_in_a_gap(where):
    a, x, _ = _arena()
    a["out"].copy_(x)
    sp = {n: (s, e) for n, s, e, _, _ in a.spans}
    off, text = {"front": (sp["x"][0] - 1, "1 bytes before `x`"), "after_x": (sp["x"][1] + 5, "5 bytes past the end of `x`"),
                 "before_out": (sp["out"][0] - 256, "256 bytes before `out`"), "tail": (a.nbytes - 1, "bytes past the end of `out`")}[where]
    a.buf[a.base + off] ^= 0x10                                      # one bit: NaN stays NaN, so only an integer comparison sees it
    r = a.check()
    assert not r.ok and r.changed_bytes == 1 and f"byte {off} of the arena" in r.changed and text in r.changed, str(r)
    assert r.unwritten == {"out": 0}
    a.buf[a.base + off] ^= 0x10
    assert a.check().ok


def test_arena_reports_an_output_element_left_at_its_fill():
    a, x, _ = _arena()
    a["out"].copy_(x)
    a["out"].view(torch.int32).view(-1)[12345] = Hy.PATTERN["float32"]
    r = a.check()
    assert not r.ok and r.changed is None and r.unwritten == {"out": 1} and "1 elements of `out`" in str(r)
    a16, x16, _ = _arena("bfloat16")
    a16["out"].copy_(x16)
    a16["out"].view(torch.int16).view(-1)[-1] = Hy.PATTERN["bfloat16"]
    assert a16.check().unwritten == {"out": 1}


# ---- the plan search on the host rule

@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build(tmp_path_factory.mktemp("history_plan"))


def _plan_many(driver, t, ncu):
    return lambda shapes: [fields(p) for p, _ in driver([Hy.host_query(t, ncu, s) for s in shapes])]


@pytest.mark.parametrize("ncu", [256, 304, 64])
def test_search_reaches_every_structure(driver, ncu):
    """At 256 CUs (the MI355X) every listed structure is reached under the cap - a condition; so it is at 304 and at 64 (a partition)."""
    found = {}
    for t in Hy.TARGETS:
        s = Hy.find_shape(t, _plan_many(driver, t, ncu), ncu, Hy.host_ignore(t))
        assert s is not None, (ncu, t.name)
        pl = fields(driver([Hy.host_query(t, ncu, s)])[0][0])
        assert Hy.matches(t, pl, ncu, Hy.host_ignore(t)) and pl["structure"] == t.structure
        assert pl["chains"] == Hy.chains_of(*s) <= Hy.shape_cap(ncu)
        found[t.name] = (s, pl["chains"])
    print(f"ncu {ncu}: " + ", ".join(f"{k} {s[0]}x{s[1]}x{s[2]} ({c} chains)" for k, (s, c) in found.items()))
    assert {t.structure for t in Hy.TARGETS} >= {"small2", "small3", "mid4", "chain2", "chain2_split", "chain2_sf0", "split16_4", "split16_3",
                                                 "winograd_ws3", "winograd_ws4", "direct4", "bf16_mid4", "bf16_3", "bf16_3_split", "bf16_4"}
    if ncu == 256:                                                   # what the search finds on the MI355X's rule (recorded: the GPU test prints the same)
        assert found["small2"][0] == (1, 36, 136) and found["mid4"][0] == (1, 68, 136)
        assert found["chain2-mfma32"][0] == (4, 68, 136) and found["chain2_split"][0] == (6, 68, 136) and found["chain2-mfma16"][0] == (9, 68, 136)


def test_named_starting_points_at_256_cus(driver):
    """The shapes the work item names for a 256-CU device - 64x128 with 1 / 5 / 8 / 9 clips, and 16x24 - give mid4 (224 tiles, 32 chains),
    chain2 on 32x32x16 (160 chains), chain2 on 16x16x32 (256 chains), chain2_split (288 chains) and small2 under the host rule."""
    want = [((1, 64, 128), "mid4", 32, 32), ((5, 64, 128), "chain2", 160, 32), ((8, 64, 128), "chain2", 256, 16), ((9, 64, 128), "chain2_split", 288, 32),
            ((1, 16, 24), "small2", 2, 32)]
    got = [fields(p) for p, _ in driver([f"256 7 {B} {H} {W} {H} 1" for (B, H, W), _, _, _ in want])]
    for (shape, name, chains, mfma), pl in zip(want, got):
        assert (pl["structure"], pl["chains"], pl["mfma"]) == (name, chains, mfma), (shape, pl)
    assert got[0]["tiles"] == 224


def test_candidates_order_and_cap():
    c = Hy.candidates(256)
    assert c[0] == (1, 68, 136) and c[:9] == [(1, H, 136) for H in range(68, 0, -8)]
    assert all(H % 2 == 0 and H % 8 == 4 and W % 32 == 8 for _, H, W in c)          # every shape ragged in both directions, even
    assert max(Hy.chains_of(*s) for s in c) <= Hy.shape_cap(256) == 640
    assert Hy.persistent_grid(7) == 8 and Hy.persistent_grid(255) == 248 and Hy.persistent_grid(304) == 304
    assert [t.name for t in Hy.family_targets()] == ["small2", "mid4", "chain2-mfma16", "chain2_split", "winograd_ws3", "bf16_3"]
    assert (Hy.FLOOD_DH % 8, Hy.FLOOD_DW % 32) != (0, 0) and Hy.FLOOD_DH % 2 == 0 and Hy.FLOOD_DW % 2 == 0
