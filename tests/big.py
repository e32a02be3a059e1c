"""Arithmetic of the large-tensor tests (tests/test_gpu_big.py): how many items of a tiny frame carry one tensor past a byte or element
threshold, which items sit at the threshold, what a case costs in device memory, and the non-local block's batch at its chunk limit.
Nothing here touches a GPU; tests/test_big_host.py pins the numbers.

A *tier* is a threshold one tensor of a call must cross: its last byte (element) lies at or beyond the threshold and at least one whole
item lies beyond it.
  A  byte offset 2^31   signed 32-bit byte arithmetic, the buffer resources' out-of-range offset 0x7fffffff
  B  byte offset 2^32   unsigned wrap, a buffer resource's num_records
  C  element index 2^31 the flat kernels
  N  more than 65535 items: kernels that carry the item in gridDim.y / gridDim.z
  E  byte offset 2^33 of an fp32 tensor = element index 2^31.  At tier B an fp32 tensor has 2^30 elements: a 32-bit BYTE offset wraps
     there, an `int` ELEMENT product (item * H * W * 64 without its size_t) does not.  It wraps here; a few one-input hooks run at it.
"""
from __future__ import annotations

TIER_A = 1 << 31
TIER_B = 1 << 32
TIER_C = 1 << 31              # elements, not bytes
TIER_E = 1 << 33
TIER_N = 65535                # gridDim.y / gridDim.z hold at most this many
N_ITEMS = TIER_N + 3          # 65538: past one full grid axis, and a multiple of 3

DEFAULT_HW = (33, 70)         # ragged in both axes: 5 x 3 tiles of 8 x 32
T = 3                         # the fewest frames per chain, so the most chains per byte
MAX_CASE_BYTES = 40 << 30     # no case may need more
NL_CHUNK_LIMIT = 0x7fff0000   # bytes of packed operands one launch of nl_attn_f16_sw_kernel addresses (nonlocal_f16.hip)
NL_F16_CP = 96                # NF_CP, the padded channel count of its packed operands


def item_bytes(bpp: int, H: int, W: int) -> int:
    return bpp * H * W


def items_for(bpp: int, H: int, W: int, frames: int = T, threshold: int = TIER_B) -> int:
    """The fewest items (a whole number of chains of ``frames``) of ``bpp`` bytes per pixel whose tensor crosses ``threshold``: the item
    holding the threshold and one whole item beyond it."""
    n = threshold // item_bytes(bpp, H, W) + 2
    return -(-n // frames) * frames


def crosses(bpp: int, H: int, W: int, items: int, threshold: int) -> bool:
    """At least one whole item of the tensor lies at or beyond ``threshold``."""
    return (items - 1) * item_bytes(bpp, H, W) >= threshold


def straddlers(bpp: int, H: int, W: int, items: int, thresholds=(TIER_A, TIER_B, TIER_E)) -> dict:
    """{threshold: (last item wholly below, the item holding the threshold's byte, first item wholly above)} for every threshold the
    tensor of ``items`` items crosses."""
    ib = item_bytes(bpp, H, W)
    out = {}
    for th in thresholds:
        if not crosses(bpp, H, W, items, th):
            continue
        k = th // ib                                   # item k holds byte `th`
        below = k - 1                                  # ends at or before the threshold either way
        above = k + 1 if k * ib < th else k            # an item that starts exactly at the threshold is wholly above it
        out[th] = (below, k, above)
    return out


def selected_items(bpp: int, H: int, W: int, items: int, thresholds=(TIER_A, TIER_B, TIER_E)) -> list:
    """The items a case compares with the fp64 spec: the straddlers of every crossed threshold, the first item and the last."""
    sel = {0, items - 1}
    for tri in straddlers(bpp, H, W, items, thresholds).values():
        sel.update(i for i in tri if 0 <= i < items)
    return sorted(sel)


def footprint(tensor_bytes, staging: int = 0, parts_bytes: int = 0) -> int:
    """Device bytes of one case: its tensors, what the hook stages beside them, and the outputs of the largest slice of the parts run."""
    return int(sum(tensor_bytes) + staging + parts_bytes)


def slices(units: int, unit_bytes: int, limit: int = TIER_A) -> list:
    """[(u0, u1)] covering 0 .. units in the fewest equal runs of whole units, each run below ``limit`` bytes of its largest tensor
    (``unit_bytes`` per unit)."""
    per = max(1, (limit - 1) // unit_bytes)
    n = -(-units // per)
    per = -(-units // n)
    return [(u, min(units, u + per)) for u in range(0, units, per)]


def nl_npad(N: int) -> int:
    return (N + 31) // 32 * 32 + 64


def nl_f16_scratch_halfs(B: int, N: int) -> int:
    """nl_f16_scratch_halfs of nonlocal_f16.hip: Khi, Klo, Vthi, Vtlo."""
    return 4 * B * NL_F16_CP * nl_npad(N)


def nl_max_batch_one_launch(N: int, limit: int = NL_CHUNK_LIMIT) -> int:
    """The largest B whose packed operands one launch addresses (nl_f16_fits_one_launch): 2 bytes x nl_f16_scratch_halfs(1, N) x B <= limit."""
    return limit // (2 * nl_f16_scratch_halfs(1, N))


def nl_padded_ch(C: int) -> int:
    return 32 * ((C + 31) // 32)
