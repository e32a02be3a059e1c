"""The launch plan (pfnl_amd/csrc/launch_plan.h: Options, trunk_plan, plan_text) on the host (no GPU), compiled into a small driver with
hipcc (tests/plan_driver.py): the rule reproduces the table recorded from the library on the 256-CU MI355X, the plan expectations the GPU
tests state, and its invariants at CU counts from 0 to 304."""
import gzip
import os
import random

import pytest

from conftest import ROOT
from plan_driver import build, fields, nl_fits_of

TABLE = os.path.join(ROOT, "tests", "golden", "plan_table_cu256.txt.gz")

# every single-option change of the recorded table (and of the invariants below)
SETTINGS = [(), ("strict_fp32=on",), ("precision=bf16",), ("precision=bf16", "bf16_conv10=separate"), ("precision=bf16", "bf16_mfma=32")]
SETTINGS += [(f"conv3x3={v}",) for v in ("winograd", "winograd_tile", "direct", "split16", "auto")]
SETTINGS += [("small=on",), ("small=off",), ("small_c10=off",)]
SETTINGS += [(k + "=off",) for k in ("split16_chain", "split16_c10", "split16_sf", "split16_mid", "split16_splitchains")]
SETTINGS += [("split16_sf0=on",), ("split16_mfma=32",), ("merge1=winograd",), ("conv2=split",), ("conv1x1=stream",), ("nonlocal=f32",),
             ("nonlocal=split16",)]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build(tmp_path_factory.mktemp("plan_host"))


def grid_of(ncu):
    """persistent_grid: the CU count rounded down to whole XCDs, at least 8."""
    return max(8, ncu // 8 * 8)


def cuts(chains, T, G):
    """split_rule (chain_order.h): a last, partial round of R chains is cut when at least two parts of a chain fit the idle workgroups."""
    R = chains % G
    return chains > G and 0 < R <= G // 2 and min(T, G // R) >= 2


def chains_of(B, H, W):
    return B * ((W + 31) // 32) * ((H + 7) // 8)


def plans(driver, cases, ncu=256):
    """cases: (T, B, H, W, "key=value ...") -> the plan of each as a dict (nl_fits = 1: no shape of these tests is beyond one launch)."""
    return [fields(p) for p, _ in driver([f"{ncu} {T} {B} {H} {W} {H} 1 {opts}" for T, B, H, W, opts in cases])]


def test_reproduces_the_table_recorded_on_256_cus(driver):
    """tests/golden/plan_table_cu256.txt.gz (text, gzipped: 830 KB of near-identical lines), one line per case: "T B H W key=value ... |
    pfnl_plan text", recorded from the library on the MI355X (256 CUs) before the rule moved into launch_plan.h - T 5 / 7, 1 - 9 clips,
    seven shapes from 32x32 to 270x480, the defaults and every SETTINGS entry.  `zcat` shows it."""
    with gzip.open(TABLE, "rt") as f:
        rows = [line.rstrip("\n").split(" | ") for line in f if line.strip()]
    assert len(rows) == 2 * 9 * 7 * len(SETTINGS)
    queries = []
    for inputs, text in rows:
        T, B, H, W, *opts = inputs.split()
        queries.append(" ".join(["256", T, B, H, W, H, str(nl_fits_of(text))] + opts))
    assert {tuple(q.split()[7:]) for q in queries} == set(SETTINGS)
    got = driver(queries)
    bad = [(q, g[0], r[1]) for q, g, r in zip(queries, got, rows) if g[0] != r[1]]
    assert not bad, f"{len(bad)} of {len(rows)} plans differ, e.g. (query, header, recorded) = {bad[:2]}"


def test_pinned_cases(driver):
    """By hand from the rule, 256 CUs, T = 7."""
    small, mid, chain, strict, bf = plans(driver, [(7, 1, 32, 32, ""), (7, 1, 128, 128, ""), (7, 4, 128, 128, ""), (7, 4, 128, 128, "strict_fp32=on"),
                                                   (7, 4, 128, 128, "precision=bf16")])
    assert (small["structure"], small["launches_per_block"], small["merge1"]) == ("small2", 2, "small")
    assert (mid["structure"], mid["launches_per_block"], mid["mfma"]) == ("mid4", 4, 32)
    assert (chain["structure"], chain["launches_per_block"], chain["mfma"], chain["c1_mfma"], chain["merge1"]) == ("chain2", 2, 16, 16, "split16")
    assert (strict["structure"], strict["conv1x1"], strict["merge1"]) == ("winograd_ws3", "stream", "winograd")
    assert (bf["structure"], bf["mfma"], bf["merge1"]) == ("bf16_3", 16, "bf16")


# ---- the plan expectations of the GPU tests, at the MI355X's 256 CUs and the same shapes

def test_gpu_expectation_harness_shapes(driver):
    """test_gpu_forward.test_harness_two_in_flight_is_byte_identical"""
    for pl in plans(driver, [(7, 1, 144, 180, ""), (7, 1, 12, 20, ""), (7, 1, 96, 128, "")]):
        assert pl["structure"] in ("mid4", "small2")


def test_gpu_expectation_sf0(driver):
    """test_gpu_forward.test_forward_sf0_is_bit_identical"""
    for T, B, H, W in [(7, 3, 128, 128), (7, 4, 128, 128), (7, 3, 100, 130), (5, 5, 96, 128), (3, 6, 90, 98), (7, 1, 270, 480)]:
        off, on = plans(driver, [(T, B, H, W, "split16_mfma=32"), (T, B, H, W, "split16_mfma=32 split16_sf0=on")])
        assert off["structure"] in ("chain2", "chain2_split") and off["sf0"] == 0, off
        assert on["structure"] == "chain2_sf0" and on["launches_per_block"] == 2 + on["c1x1"] and on["sf0"] == 1, on


def test_gpu_expectation_chain_mfma_shapes(driver):
    """test_gpu_forward.test_chain_launch_mfma_shapes and test_gpu_c1c10_mfma16.test_forward_c1c10_mfma16"""
    shapes = ((4, 128, 128), (2, 180, 318), (1, 180, 318), (5, 128, 128), (1, 64, 64))
    got = plans(driver, [(7, B, H, W, "") for B, H, W in shapes])
    assert [pl["mfma"] for pl in got] == [16, 16, 32, 32, 32]
    for (B, H, W), pl in zip(shapes, got):
        chains = chains_of(B, H, W)
        assert pl["mfma"] == (16 if chains >= 256 and not cuts(chains, 7, 256) else 32), (B, H, W, pl)
        assert pl["c1_mfma"] == pl["mfma"]
    for pl in plans(driver, [(7, B, H, W, "split16_mfma=32") for B, H, W in shapes]):
        assert pl["mfma"] == 32 and pl["c1_mfma"] == 32, pl
    for pl in plans(driver, [(7, 4, 128, 128, ""), (7, 2, 180, 318, "")]):
        assert pl["c1_mfma"] == 16, pl


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_gpu_expectation_split_chains(driver, prec):
    """test_gpu_forward.test_forward_split_chains and test_gpu_bf16.test_forward_bf16_split_chains"""
    G = 256
    opt = "" if prec == "fp32" else "precision=bf16"
    whole, cut_name = ("chain2", "chain2_split") if prec == "fp32" else ("bf16_3", "bf16_3_split")
    params = {"fp32": [(7, 128, 128, (4, 5, 6, 7, 9)), (7, 100, 130, (5, 9)), (5, 96, 128, (7,)), (3, 90, 98, (11,))],
              "bf16": [(7, 128, 128, (4, 5, 6, 9)), (7, 100, 130, (5,)), (5, 96, 128, (7,)), (3, 90, 98, (11,))]}[prec]
    ncut = 0
    for T, H, W, Bs in params:
        for B in Bs:
            pl, off = plans(driver, [(T, B, H, W, opt), (T, B, H, W, opt + " split16_splitchains=off")])
            chains = chains_of(B, H, W)
            R = chains % G
            cut = cuts(chains, T, G)
            ncut += cut
            assert pl["structure"] == (cut_name if cut else whole), (B, pl)
            assert off["structure"] == whole
            if cut:
                assert pl["launches_per_block"] == (3 if prec == "fp32" else 4) and pl["c1x1"] == 1
                assert pl["whole_chains"] == chains - R and pl["split_parts"] * pl["part_frames"] >= T > (pl["split_parts"] - 1) * pl["part_frames"]
                assert (chains - pl["whole_chains"]) * pl["split_parts"] <= G
    assert ncut >= 4


def test_gpu_expectation_plan_is_what_runs(driver):
    """test_gpu_forward.test_plan_is_what_runs"""
    cases = [((1, 32, 32), "", "small2", "small"), ((1, 32, 32), "small_c10=off", "small3", "small"), ((1, 128, 128), "", "mid4", "split16"),
             ((1, 128, 128), "split16_mid=off", "chain2", "split16"), ((3, 128, 128), "", "chain2", "split16"),
             ((5, 128, 128), "", "chain2_split", "split16_cut"), ((3, 128, 128), "merge1=winograd", "chain2", "winograd"),
             ((3, 128, 128), "split16_sf0=on", "chain2_sf0", "split16"), ((3, 128, 128), "split16_c10=off", "split16_3", "split16"),
             ((3, 128, 128), "split16_chain=off", "split16_3", "split16"), ((3, 128, 128), "split16_sf=off", "split16_4", "split16"),
             ((3, 128, 128), "strict_fp32=on", "winograd_ws3", "winograd"),
             ((1, 64, 64), "conv3x3=direct conv1x1=tiled small=off", "direct4", "direct"),
             ((1, 64, 64), "conv3x3=winograd small=off", "winograd_ws4", "direct"),
             ((3, 128, 128), "precision=bf16", "bf16_3", "bf16"), ((5, 128, 128), "precision=bf16", "bf16_3_split", "bf16"),
             ((1, 128, 128), "precision=bf16", "bf16_mid4", "bf16"), ((3, 128, 128), "precision=bf16 bf16_conv10=separate", "bf16_4", "bf16")]
    got = plans(driver, [(7, B, H, W, opts) for (B, H, W), opts, _, _ in cases])
    for ((B, H, W), opts, want, merge1), pl in zip(cases, got):
        assert pl["structure"] == want and pl["merge1"] == merge1, (B, H, W, opts, pl)
        assert pl["tiles"] == B * 7 * ((W + 31) // 32) * ((H + 7) // 8) and pl["chains"] == pl["tiles"] // 7


# ---- invariants at other CU counts

# structure -> (launches per block, of them class conv1x1); None: depends on the plan, checked below
LAUNCHES = {"small2": (2, 0), "small3": (3, 1), "mid4": (4, 1), "chain2": (2, 0), "chain2_split": (3, 1), "chain2_sf0": None, "split16_3": None,
            "split16_4": (4, 1), "winograd_ws3": (3, 1), "winograd_ws4": (4, 1), "winograd_tile4": (4, 1), "direct4": (4, 1),
            "bf16_mid4": (4, 1), "bf16_3": (3, 0), "bf16_3_split": (4, 1), "bf16_4": (4, 1)}


def test_invariants_at_any_cu_count(driver):
    rng = random.Random(20)
    shapes = [(rng.randint(1, 12), 2 * rng.randint(1, 256), 2 * rng.randint(1, 256)) for _ in range(240)]
    ncus = [0, 1, 7] + list(range(8, 305, 8))
    queries = []
    for i, (B, H, W) in enumerate(shapes):
        for T in (3, 5, 7):
            for j, opts in enumerate(SETTINGS):
                # under the defaults every CU count; under a changed option six of them, another six for the next shape and setting
                for ncu in ncus if not opts else [ncus[(7 * k + i + j) % len(ncus)] for k in range(6)]:
                    queries.append(f"{ncu} {T} {B} {H} {W} {H} 1 " + " ".join(opts))
    got = driver(queries)
    assert got == driver(queries), "the same inputs give another plan"
    seen = set()
    for q, (text, extras) in zip(queries, got):
        ncu, T = (int(v) for v in q.split()[:2])
        pl, ex, G = fields(text), fields(extras), grid_of(ncu)
        name, fp32 = pl["structure"], pl["precision"] == "fp32"
        seen.add(name)
        ctx = (q, text, extras)
        s = pl["split_parts"]
        if s > 0:
            assert pl["whole_chains"] % G == 0 and 0 < pl["whole_chains"] < pl["chains"] and 2 <= s <= 7, ctx
        else:
            assert pl["whole_chains"] == pl["chains"], ctx
        if fp32:
            if pl["mfma"] == 16:
                assert pl["c10_fused"] and pl["chain"] and not pl["sf0"] and not s and pl["chains"] >= G, ctx
            if pl["conv3x3"] == "small":
                assert not ex["mid"] and not pl["chain"] and not pl["c10_fused"] and name in ("small2", "small3"), ctx
        want = LAUNCHES[name]
        if name == "chain2_sf0":
            want = (3, 1) if s else (2, 0)
        elif name == "split16_3":
            want = (3, 0 if pl["c10_fused"] else 1)
        assert (pl["launches_per_block"], pl["c1x1"]) == want, ctx
        assert ex["mid"] == (name in ("mid4", "bf16_mid4")), ctx
        assert (ex["p10_floats"] != 0) == bool(ex["small_c10"]) and ex["small_c10"] == (name == "small2"), ctx
        assert (ex["inp0sf_floats"] != 0) == bool(fp32 and pl["sf0"]), ctx
        assert (ex["c10part_floats"] != 0) == (s > 0), ctx
        assert (ex["merge_stride"] == 48) == (pl["merge1"] == "direct") and ex["merge_stride"] in (48, 64), ctx
    assert seen == set(LAUNCHES), set(LAUNCHES) - seen                 # the sweep reaches every structure
