"""pfnl_amd/csrc/chain_order.h on the host (no GPU), compiled into a small driver with hipcc: the work order of the persistent 3x3 launches
(every workgroup's share walked tile by tile), the trunk plan's split rule and the one geometry check every split launcher applies."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

DRIVER = r"""
#include <cstdio>
#include <vector>
#include "chain_order.h"

// every workgroup of a launch of `grid` over `nchains` chains of T frames: "ok" or the first broken property
template <bool SPLIT, int LEAD>
const char* walk(int nchains, int T, int grid, int n_full, int split_s, int split_q) {
    std::vector<int> seen((size_t)nchains * T, 0), heads(nchains, 0);
    const int L = T + LEAD;
    for (unsigned bx = 0; bx < (unsigned)grid; ++bx) {
        pfnl::ChainShare<SPLIT, LEAD> cs(bx & 7, bx >> 3, (unsigned)grid >> 3, nchains, n_full);
        if (cs.idle()) continue;
        cs.deal(L, split_s, split_q);
        if (cs.nt <= 0) continue;
        int ch0, pos0;
        cs.tile(0, L, ch0, pos0);
        if (pos0 != cs.head_pos(0)) return "first tile not at head_pos(0)";
        if (SPLIT && cs.nfc == 0 && cs.has_part && pos0 != (LEAD ? 0 : cs.sp_f0)) return "part-only workgroup does not start at its f0";
        int pos = cs.head_pos(0), tiles = 0;
        for (int k = 0; k < cs.nt; ++k) {
            int ch, p;
            cs.tile(k, L, ch, p);
            if (ch < 0 || ch >= nchains || p < 0 || p >= L) return "tile outside the chains";
            if (p != pos) return "position does not follow the walk";
            if (p < LEAD) ++heads[ch];
            else if (++seen[(size_t)ch * T + p - LEAD] > 1) return "(chain, frame) covered twice";
            pos = p + 1 == cs.end_pos(k, L) ? cs.head_pos(k + 1) : p + 1;
            if (LEAD && SPLIT && k == cs.nfull_tiles) pos = cs.sp_f0 + 1;       // a part: its shared half, then its frames
            ++tiles;
        }
        if (SPLIT && cs.has_part && cs.slot % split_s == 0 && cs.sp_f0 != 0) return "part 0 does not start at frame 0";
        (void)tiles;
    }
    for (size_t i = 0; i < seen.size(); ++i)
        if (seen[i] != 1) return "(chain, frame) not covered";
    if (LEAD)
        for (int ch = 0; ch < nchains; ++ch)
            if (heads[ch] != (ch < n_full || !SPLIT ? 1 : split_s)) return "shared half missing from a chain or a part";
    return "ok";
}

// stdin: "g H W items T n_full split_s split_q grid" -> 0 / 1 (split_geometry_ok); "r chains T grid" -> "n_full s q" or "-" (split_rule);
// "w lead nchains T grid n_full split_s split_q" (split_s = 0: no split chains) -> walk()
int main() {
    char op;
    while (std::scanf(" %c", &op) == 1) {
        if (op == 'w') {
            int lead, nchains, T, grid, n_full, s, q;
            if (std::scanf("%d %d %d %d %d %d %d", &lead, &nchains, &T, &grid, &n_full, &s, &q) != 7) return 2;
            const char* r = s == 0 ? (lead ? walk<false, 1>(nchains, T, grid, 0, 0, 0) : walk<false, 0>(nchains, T, grid, 0, 0, 0))
                                   : (lead ? walk<true, 1>(nchains, T, grid, n_full, s, q) : walk<true, 0>(nchains, T, grid, n_full, s, q));
            std::printf("%s\n", r);
        } else if (op == 'g') {
            int H, W, items, T, n_full, s, q, grid;
            if (std::scanf("%d %d %d %d %d %d %d %d", &H, &W, &items, &T, &n_full, &s, &q, &grid) != 8) return 2;
            std::printf("%d\n", pfnl::split_geometry_ok(H, W, items, T, n_full, s, q, grid) ? 1 : 0);
        } else {
            int chains, T, grid, n_full = -1, s = -1, q = -1;
            if (std::scanf("%d %d %d", &chains, &T, &grid) != 3) return 2;
            if (pfnl::split_rule(chains, T, grid, n_full, s, q)) std::printf("%d %d %d\n", n_full, s, q);
            else std::printf("-\n");
        }
    }
    return 0;
}
"""

TS = (3, 5, 7)
GRIDS = range(8, 257, 8)


def chain_counts(grid):
    """From below one round of the grid to several rounds, with the edges of every round."""
    return sorted({1, grid // 2, grid - 1, grid, grid + 1, grid + grid // 8, grid + grid // 2, 2 * grid - 1, 2 * grid, 2 * grid + 3,
                   3 * grid + grid // 4, 4 * grid + 1} - {0})


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("chain_order")
    src, exe = d / "driver.cpp", d / "driver"
    src.write_text(DRIVER)
    r = subprocess.run([hipcc, "-O1", "-std=c++17", "-I", os.path.join(ROOT, "pfnl_amd", "csrc"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr

    def run(queries):
        out = subprocess.run([str(exe)], input="\n".join(queries) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
        assert len(out) == len(queries) + 1
        return out[:-1]

    return run


def geometry_ok(nchains, T, n_full, s, q, grid):
    """The split geometry the kernels assume: whole rounds of the grid in front, behind them s <= 7 non-empty parts of <= q frames that
    together are the T frames, one part per workgroup."""
    if n_full < 0 or n_full % grid or n_full >= nchains or not 2 <= s <= 7 or q < 1:
        return False
    parts = [range(r * q, min(T, (r + 1) * q)) for r in range(s)]
    if any(len(p) == 0 for p in parts) or sorted(f for p in parts for f in p) != list(range(T)):
        return False
    return (nchains - n_full) * s <= grid


def test_split_geometry_ok_accepts_exactly_the_geometries_the_kernels_assume(driver):
    cases = []
    for T in TS + (9,):                                                         # (T = 9: nine parts of one frame are refused, > 7)
        for grid in GRIDS:
            for nchains in chain_counts(grid):
                for n_full in sorted({-grid, 0, grid, nchains - nchains % grid, nchains - nchains % grid + grid, 1}):
                    for s in range(1, 10):
                        for q in range(0, T + 2):
                            cases.append((nchains, T, n_full, s, q, grid))
    # nchains chains as one row of 32-pixel tiles of one clip-row: H = 8, W = 32 nchains, items = T (and a ragged last tile)
    got = driver([f"g 8 {32 * c - 5} {T} {T} {n} {s} {q} {g}" for c, T, n, s, q, g in cases])
    bad = [c for c, v in zip(cases, got) if (v == "1") != geometry_ok(*c)]
    assert not bad, f"{len(bad)} of {len(cases)} geometries judged wrongly, e.g. (chains, T, n_full, s, q, grid) = {bad[:5]}"
    assert sum(v == "1" for v in got) > 1000                                    # the sweep reaches the accepted geometries


def split_rule(chains, T, grid):
    """The trunk plan's rule: R = chains mod grid chains of a last, partial round are cut when two or more parts fit the idle workgroups."""
    R = chains % grid
    if T > 7 or chains <= grid or R == 0 or grid // R < 2:
        return None
    s0 = min(T, grid // R)
    q = -(-T // s0)
    s = -(-T // q)
    return (chains - R, s, q) if s >= 2 else None


def test_split_rule_outputs_pass_the_check(driver):
    cases = [(c, T, g) for T in TS + (8,) for g in GRIDS for c in chain_counts(g)]
    got = driver([f"r {c} {T} {g}" for c, T, g in cases])
    cuts = []
    for (chains, T, grid), v in zip(cases, got):
        want = split_rule(chains, T, grid)
        assert v == ("-" if want is None else "%d %d %d" % want), (chains, T, grid, v)
        if want is not None:
            assert geometry_ok(chains, T, *want, grid), (chains, T, grid, want)
            cuts.append(f"g 8 {32 * chains} {T} {T} {want[0]} {want[1]} {want[2]} {grid}")
    assert len(cuts) > 100 and driver(cuts) == ["1"] * len(cuts)


def test_split_rule_pinned_cases(driver):
    # 5 clips of 128 x 128 on 256 workgroups: 320 chains = 1.25 rounds -> the last 64 chains in 4 parts of 2 frames (T = 7)
    assert driver(["r 320 7 256", "r 256 7 256", "r 512 7 256", "r 300 7 256", "r 320 9 256"]) == ["256 4 2", "-", "-", "256 4 2", "-"]
    # by hand on grids that are not powers of two: 300 chains of 5 frames on 248 -> R = 52, 4 fit: q = 2, 3 parts; 330 of 3 on 304 -> R = 26,
    # 11 fit: 3 parts of 1; 200 of 7 on 120 -> R = 80, only 1 fits: no cut; 250 of 2 on 240 -> R = 10: 2 parts of 1
    assert driver(["r 300 5 248", "r 330 3 304", "r 200 7 120", "r 250 2 240"]) == ["248 3 2", "304 3 1", "-", "240 2 1"]


def test_work_order_covers_every_frame_once(driver):
    """Over all workgroups every (chain, frame) exactly once; with lead = 1 every chain and every part holds the shared-half tile; each
    workgroup's first tile at head_pos(0), a workgroup without whole chains at its part's f0 (the convmerge1 case); the tile decode and
    the increments the kernels make (end_pos / head_pos) agree."""
    cases = []
    for T in TS:
        for grid in GRIDS:
            for nchains in chain_counts(grid):
                for lead in (0, 1):
                    cases.append((lead, nchains, T, grid, 0, 0, 0))
                    R = nchains % grid
                    for n_full in {nchains - R, nchains - R - grid} if R else ():
                        if n_full < 0:
                            continue
                        for s in range(2, 8):
                            for q in range(1, T + 1):
                                if geometry_ok(nchains, T, n_full, s, q, grid):
                                    cases.append((lead, nchains, T, grid, n_full, s, q))
    got = driver(["w " + " ".join(map(str, c)) for c in cases])
    bad = [(c, v) for c, v in zip(cases, got) if v != "ok"]
    assert not bad, f"{len(bad)} of {len(cases)} launches broken, e.g. (lead, chains, T, grid, n_full, s, q) = {bad[:3]}"
    assert sum(c[5] > 0 and c[4] == 0 for c in cases) > 10                   # n_full = 0 (part-only workgroups) is in the sweep
