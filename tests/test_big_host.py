"""The arithmetic of tests/big.py, which sizes the large-tensor GPU tests (tests/test_gpu_big.py): item counts, the items at the
thresholds, the non-local batch at the real chunk limit, footprints.  No GPU."""
import os
import re

import big

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "pfnl_amd", "csrc")


def test_fp32_item_counts_and_straddlers():
    H, W = big.DEFAULT_HW
    assert big.item_bytes(256, H, W) == 591360
    assert big.items_for(256, H, W, 3, big.TIER_B) == 7266                       # 2422 chains of T = 3
    assert 7266 * 591360 == 4296821760                                           # the 4.30 GB tensor
    s = big.straddlers(256, H, W, 7266)
    assert s[big.TIER_A] == (3630, 3631, 3632)
    assert s[big.TIER_B] == (7261, 7262, 7263)
    assert big.selected_items(256, H, W, 7266) == [0, 3630, 3631, 3632, 7261, 7262, 7263, 7265]


def test_128_bytes_per_pixel_doubles_the_indices():
    H, W = big.DEFAULT_HW
    n = 2 * big.items_for(256, H, W, 3, big.TIER_B)
    assert n == 14532 and n % 3 == 0
    assert n >= big.items_for(128, H, W, 3, big.TIER_B) and big.crosses(128, H, W, n, big.TIER_B)
    s = big.straddlers(128, H, W, n)
    assert s[big.TIER_A] == (7261, 7262, 7263) and s[big.TIER_B] == (14524, 14525, 14526)


def test_straddlers_are_below_holding_above_for_every_crossed_threshold():
    for bpp, H, W in ((256, 33, 70), (128, 33, 70), (256, 34, 70), (12, 2, 2), (4, 1, 1), (256, 8, 32), (256, 32, 32)):
        ib = bpp * H * W
        for th in (big.TIER_A, big.TIER_B):
            for frames in (1, 3, 7):
                n = big.items_for(bpp, H, W, frames, th)
                assert n % frames == 0 and big.crosses(bpp, H, W, n, th) and n - frames < th // ib + 2   # and no chain to spare
                s = big.straddlers(bpp, H, W, n)
                assert th in s and (th == big.TIER_A or big.TIER_A in s)          # a tier-B tensor crosses A as well
                lo, mid, hi = s[th]
                assert (lo + 1) * ib <= th                                       # wholly below
                assert mid * ib <= th < (mid + 1) * ib                           # holds the threshold's byte
                assert hi * ib >= th and hi < n                                  # wholly above, and inside the tensor
                assert hi - lo <= 2
                sel = big.selected_items(bpp, H, W, n)
                assert {0, n - 1, lo, mid, hi} <= set(sel) and sel == sorted(set(sel))
    assert big.straddlers(256, 33, 70, 3000) == {}                               # crosses nothing
    assert list(big.straddlers(256, 33, 70, 4000)) == [big.TIER_A]


def test_exact_multiple_threshold():
    s = big.straddlers(256, 32, 32, big.items_for(256, 32, 32, 3, big.TIER_B))   # 2^18-byte items: the threshold is an item boundary
    assert s[big.TIER_B] == (16383, 16384, 16384)


def test_slices_cover_in_whole_units_below_the_limit():
    for units, ub in ((2422, 3 * 591360), (4844, 3 * 295680), (5465, 3 * 32 * 32 * 256), (7, 100)):
        sl = big.slices(units, ub)
        assert sl[0][0] == 0 and sl[-1][1] == units and all(a[1] == b[0] for a, b in zip(sl, sl[1:]))
        assert all(0 < (u1 - u0) * ub < big.TIER_A for u0, u1 in sl)
    assert len(big.slices(2422, 3 * 591360)) == 3


def test_nonlocal_batch_at_the_real_chunk_limit():
    """T = 3, LR 8 x 16: N = 32 keys, npad = 96; one clip's packed operands are 4 arrays x 96 channels x 96 keys of 2 bytes."""
    N = (8 // 2) * (16 // 2)
    assert N == 32 and big.nl_npad(N) == 96
    assert 2 * big.nl_f16_scratch_halfs(1, N) == 73728
    B = big.nl_max_batch_one_launch(N)
    assert B == 29126
    assert 2 * big.nl_f16_scratch_halfs(B, N) <= big.NL_CHUNK_LIMIT < 2 * big.nl_f16_scratch_halfs(B + 1, N)
    assert big.NL_CHUNK_LIMIT - 2 * big.nl_f16_scratch_halfs(B, N) < 73728       # offsets run up to within a clip of the limit
    assert 2 * big.nl_f16_scratch_halfs(B, N) >= big.TIER_A - (1 << 16) - 73728  # ... which is 64 KB under the out-of-range offset
    assert B < big.TIER_N                                                        # the batch rides in gridDim.y


def test_constants_match_the_kernels_source():
    """The limit, the padded channel count and the scratch formula are restated in big.py: hold them to nonlocal_f16.hip."""
    src = open(os.path.join(CSRC, "nonlocal_f16.hip")).read()
    assert re.search(r"constexpr int NF_CP = (\d+);", src).group(1) == str(big.NL_F16_CP)
    assert "(size_t)0x7fff0000ull" in src and big.NL_CHUNK_LIMIT == 0x7fff0000
    assert "(size_t)(N + 31) / 32 * 32 + 64" in src and "return 4 * (size_t)B * NF_CP * npad;" in src


def test_footprints():
    H, W = big.DEFAULT_HW
    one = 7266 * big.item_bytes(256, H, W)
    assert big.footprint([one, one]) == 2 * one
    # the fused chain launch: x, resid, out of 7266 items, base of 2422; the hook stages x and base in the split format (128 B per pixel)
    fp = big.footprint([one, one, one, one // 3], staging=one // 2 + one // 6, parts_bytes=one // 3 + 591360)
    assert fp == 3 * one + one // 3 + one // 2 + one // 6 + one // 3 + 591360
    assert fp < big.MAX_CASE_BYTES
    assert 8 * big.TIER_B < big.MAX_CASE_BYTES                                    # eight tensors of 2^32 bytes and the hooks' staging


def test_tier_e_is_where_an_int_element_product_wraps():
    H, W = big.DEFAULT_HW
    n = big.items_for(256, H, W, 3, big.TIER_E)
    assert n == 14529 and (n - 1) * H * W * 64 >= 2 ** 31 > 7265 * H * W * 64      # the last item's first element: past int at E, not at B
    assert big.straddlers(256, H, W, n)[big.TIER_E] == (14524, 14525, 14526)
    assert set(big.straddlers(256, H, W, n)) == {big.TIER_A, big.TIER_B, big.TIER_E}


def test_tier_n_counts():
    assert big.N_ITEMS == 65538 and big.N_ITEMS > big.TIER_N and big.N_ITEMS % 3 == 0
