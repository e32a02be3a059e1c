"""Helpers of the history-independence tests (tests/test_gpu_history.py; host tests of these helpers: tests/test_history_host.py).

A forward's bits depend on the input, the weights, the options and the device - not on what the handle ran before (DESIGN.md "What a
forward may depend on").  The handle's workspace only grows, its bytes change meaning from call to call (fp32 / bf16, merge stride 48 /
64, split-chain partial slots, key-split partials, padded non-local rows), and the hot kernels let the buffer range check zero-fill what
they fetch past an operand.  Three tools to test that:

* TARGETS + find_shape: one forward per trunk structure trunk_plan (pfnl_amd/csrc/launch_plan.h) can name, at a shape found by ASKING
  the plan (PFNLEngine.plan on the device, tests/plan_driver.py on the host) - no CU-count threshold is written down here.
* the histories: functions (engine, target) that leave the handle's state as different from a fresh handle's as the public surface
  allows - non-finite floods at a larger shape, in both precisions, every other plan, a range rerun, a strip, a session.
* Arena: the operands of one call back to back inside ONE flooded allocation, so that a read past an operand meets NaN instead of
  whatever the caching allocator left next to a torch.empty, and a write past it is seen.

torch is imported where a function needs it: the module itself imports on a machine without it."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

# ---------------------------------------------------------------------------------------------------------------------------------
# targets and the plan search

W_SEARCH = 136                                   # 5 tiles of 32 columns, the last one 8 wide; even (space_to_depth)
H_SEARCH = tuple(range(68, 0, -8))               # 68, 60, ..., 12, 4: steps of 8 rows, every one 4 rows into its last tile, even
ROUNDS_CAP = 2.5                                 # the search stops at 2.5 rounds of (clip, tile) chains on the persistent grid, see shape_cap


@dataclass(frozen=True)
class Target:
    """One forward: options on top of the library's defaults, the frame count, and what the plan must say for the shape to count."""
    name: str
    structure: str
    options: Tuple[Tuple[str, str], ...] = ()
    want: Tuple[Tuple[str, object], ...] = ()    # further plan fields that must hold: ("mfma", 16), ("chains_below_grid", True), ...
    T: int = 7
    theta: bool = False                          # the weights carry the non-local block's theta / phi projections (nl_type 0)
    family: str = ""                             # small | mid | chain | chain_split | strict | bf16: the families of histories 3 - 7

    @property
    def bf16(self) -> bool:
        return ("precision", "bf16") in self.options


BF16 = (("precision", "bf16"),)
STRICT = (("strict_fp32", "on"),)

# every structure plan_fp32_trunk / plan_bf16_trunk names (winograd_tile4 is conv3x3=winograd_tile, the per-tile form of the same
# arithmetic as winograd_ws4: same buffers, same launches per block), + the general non-local family, + one T = 3 target
TARGETS: Tuple[Target, ...] = (
    Target("small2", "small2", family="small"),
    Target("small3", "small3", (("small_c10", "off"),)),
    Target("mid4", "mid4", family="mid"),
    Target("chain2-mfma32", "chain2", (), (("mfma", 32), ("chains_below_grid", True))),         # (fewer chains than the grid: the rule itself says 32)
    Target("chain2-mfma16", "chain2", (("split16_mfma", "16"),), (("mfma", 16),), family="chain"),
    Target("chain2_split", "chain2_split", (), (("merge1", "split16_cut"),), family="chain_split"),
    Target("chain2_sf0", "chain2_sf0", (("split16_sf0", "on"),)),
    Target("split16_4", "split16_4", (("split16_c10", "off"), ("split16_chain", "off"))),
    Target("split16_3", "split16_3", (("split16_c10", "off"),)),
    Target("winograd_ws3", "winograd_ws3", STRICT, family="strict"),
    Target("winograd_ws4", "winograd_ws4", STRICT),
    Target("direct4", "direct4", STRICT + (("conv3x3", "direct"),)),
    Target("bf16_mid4", "bf16_mid4", BF16),
    Target("bf16_3", "bf16_3", BF16, family="bf16"),
    Target("bf16_3_split", "bf16_3_split", BF16),
    Target("bf16_4", "bf16_4", BF16 + (("bf16_conv10", "separate"),)),
    Target("nl_sub_sample2", "small2", (("nl_sub_sample", "2"),), (("nl", "general_f32"),)),
    Target("nl_type0", "small2", (("nl_type", "0"),), (("nl", "general_f32"),), theta=True),
    Target("T3-chain2_split", "chain2_split", (), (), T=3),
)
# the only targets a device of another width may miss under the cap (their rule reads chains >= grid): reported by name with pytest.skip
MAY_BE_OUT_OF_REACH = ("chain2-mfma16", "chain2_split")

FAMILIES = ("small", "mid", "chain", "chain_split", "strict", "bf16")


def target(name: str) -> Target:
    return next(t for t in TARGETS if t.name == name)


def family_targets() -> List[Target]:
    return [next(t for t in TARGETS if t.family == f) for f in FAMILIES]


def persistent_grid(ncu: int) -> int:
    """chain_order.h persistent_grid: the CU count rounded down to whole XCDs, at least 8."""
    return ncu // 8 * 8 if ncu >= 8 else 8


def chains_of(B: int, H: int, W: int) -> int:
    return B * ((W + 31) // 32) * ((H + 7) // 8)


def shape_cap(ncu: int) -> int:
    """The largest chain count the search tries.  Every threshold of trunk_plan is a tile or chain count of at most one round of the
    persistent grid (small: 0.78 tiles per CU, mid: 0.53 chains per CU, the 16x16x32 chain kernel: chains >= grid) except the split
    rule, which needs MORE than one round with a last round R <= grid / 2: 1.5 rounds hold such a count, and an uncut partial round
    beyond one (R > grid / 2) ends below 2.  2.5 rounds leave a whole round of slack for clips that come in steps of many chains."""
    return int(ROUNDS_CAP * persistent_grid(ncu))


def candidates(ncu: int, W: int = W_SEARCH, heights: Sequence[int] = H_SEARCH) -> List[Tuple[int, int, int]]:
    """(B, H, W) in search order: B from 1, and for each B the heights from the tallest down, up to shape_cap chains.  Tall frames
    first, so that a structure is met at the fewest clips with the most keys (from 1024 keys the fp32 non-local block runs on the f16
    pipe and brings its binary16 operand buffer into play)."""
    cap = shape_cap(ncu)
    out = []
    B = 1
    while chains_of(B, min(heights), W) <= cap:
        out += [(B, H, W) for H in heights if chains_of(B, H, W) <= cap]
        B += 1
    return out


def matches(t: Target, pl: Dict[str, object], ncu: int, ignore: Sequence[str] = ()) -> bool:
    if pl.get("structure") != t.structure:
        return False
    for k, v in t.want:
        if k in ignore:
            continue
        if k == "chains_below_grid":
            if (pl["chains"] < persistent_grid(ncu)) != v:
                return False
        elif pl.get(k) != v:
            return False
    return True


def find_shape(t: Target, plan_many: Callable[[List[Tuple[int, int, int]]], List[Dict[str, object]]], ncu: int,
               ignore: Sequence[str] = ()) -> Optional[Tuple[int, int, int]]:
    """The first candidate whose plan (under t's options) is the structure wanted; None: no shape under the cap reaches it.
    plan_many: shapes -> the plan of each as a dict (the fields of pfnl_plan's text)."""
    shapes = candidates(ncu)
    for s, pl in zip(shapes, plan_many(shapes)):
        if matches(t, pl, ncu, ignore):
            return s
    return None


def host_query(t: Target, ncu: int, shape: Tuple[int, int, int]) -> str:
    """The line tests/plan_driver.py takes for this target and shape (nl_fits = 1: no candidate is beyond one launch).  nl_sub_sample is
    an integer option outside launch_plan.h's table: the driver cannot set it, and host_ignore names the plan field that then differs."""
    B, H, W = shape
    return " ".join([str(ncu), str(t.T), str(B), str(H), str(W), str(H), "1"] + [f"{k}={v}" for k, v in t.options if k != "nl_sub_sample"])


def host_ignore(t: Target) -> Tuple[str, ...]:
    return ("nl",) if any(k == "nl_sub_sample" for k, _ in t.options) else ()


# ---------------------------------------------------------------------------------------------------------------------------------
# engine plumbing

def apply_options(eng, defaults: Dict[str, str], options) -> None:
    """The library's defaults (as read from a fresh handle), then `options` on top."""
    opts = dict(defaults)
    opts.update(dict(options))
    for k, v in opts.items():
        if eng.get_option(k) != v:
            eng.set_option(k, v)


def read_defaults(eng) -> Dict[str, str]:
    return {k: eng.get_option(k) for k in eng.OPTION_KEYS}


def theta_phi(geom, w, seed=5):
    """test_gpu_forward.test_embedded_gaussian_option_forward's theta / phi variables on top of w."""
    rng = np.random.default_rng(seed)
    C = geom.nl_ch
    w = dict(w)
    for n, sc in (("theta/theta", 0.12), ("phi/phi", 0.12)):
        w[f"nlvsr/nlblock_0/{n}/kernel"] = (rng.normal(size=(1, 1, C, C)) * sc).astype(np.float32)
        w[f"nlvsr/nlblock_0/{n}/bias"] = (rng.normal(size=C) * 0.05).astype(np.float32)
    return w


def run_device(eng, x_dev):
    """A device-pointer forward of a cuda tensor, synchronised: float32 numpy."""
    import torch
    y = eng.forward(x_dev)
    torch.cuda.synchronize()
    return y.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------------------
# histories: (eng, ctx) -> None.  ctx: the target, its shape, the defaults of a fresh handle and the shapes of the other targets.

@dataclass
class Ctx:
    tgt: Target
    shape: Tuple[int, int, int]
    defaults: Dict[str, str]
    weights: Dict[str, np.ndarray]
    others: List[Tuple[Target, Tuple[int, int, int]]] = field(default_factory=list)   # history 3: (target, shape) this engine can run


FLOOD_DH, FLOOD_DW = 10, 22                      # larger than the target by no multiple of the 8 x 32 tile (and even)
FLOODS = ("nan", "inf", "noise1e4")


def flood_clip(kind: str, B: int, T: int, H: int, W: int):
    import torch
    if kind == "nan":
        return torch.full((B, T, H, W, 3), float("nan"), dtype=torch.float32, device="cuda")
    if kind == "inf":
        return torch.full((B, T, H, W, 3), float("inf"), dtype=torch.float32, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + H)
    return (torch.rand((B, T, H, W, 3), generator=g, device="cuda") * 2.0 - 1.0) * 1.0e4


def flooded(kind: str, tap: np.ndarray) -> bool:
    """The tap shows the flood: non-finite values for nan / inf; for the noise of magnitude 1e4 non-finite or far off the [0, 1]-scale
    activations of a clip (conv0 sums ~ 750 products of such inputs with Xavier weights)."""
    if not np.isfinite(tap).all():
        return True
    return kind == "noise1e4" and float(np.abs(tap).max()) > 1.0e2


def flood(eng, ctx: Ctx, kind: str, B=None, H=None, W=None) -> None:
    """History 1: a device-pointer forward of a flood clip, B + 1 clips of (H + 10) x (W + 22); the range flag is taken; the taps of
    the trunk and of convmerge1 must show the flood (else the history proves nothing)."""
    import torch
    tb, th, tw = ctx.shape
    B, H, W = B or tb + 1, H or th + FLOOD_DH, W or tw + FLOOD_DW
    x = flood_clip(kind, B, ctx.tgt.T, H, W)
    out = torch.empty(eng.out_shape(B, H, W), dtype=torch.float32, device="cuda")
    eng.forward_device(x.data_ptr(), out.data_ptr(), B, H, W)
    torch.cuda.synchronize()
    eng.range_flagged()                          # read-and-clear: the asynchronous side's flag is not left for a later call
    trunk, merge1 = eng.tap("trunk", B, H, W), eng.tap("merge1", B, H, W)
    assert flooded(kind, trunk), f"flood {kind}: the trunk tap shows none of it"
    assert flooded(kind, merge1), f"flood {kind}: the merge1 tap shows none of it"
    del x, out


def flood_other_precision(eng, ctx: Ctx, kind: str) -> None:
    """History 2: the same flood under the other of fp32 / bf16 (the library's other default plan at that shape): bf16 patterns in the
    buffers an fp32 target reads as floats, and the reverse."""
    eng.set_option("precision", "fp32" if ctx.tgt.bf16 else "bf16")
    try:
        flood(eng, ctx, kind)
    finally:
        eng.set_option("precision", "bf16" if ctx.tgt.bf16 else "fp32")


def other_plans(eng, ctx: Ctx, descending: bool) -> None:
    """History 3: every other target's options and shape on finite clips, by workspace size, ascending or descending."""
    import torch
    from pfnl_amd import synth
    order = sorted(ctx.others, key=lambda o: (o[1][0] * o[1][1] * o[1][2], o[0].name), reverse=descending)
    try:
        for i, (ot, (B, H, W)) in enumerate(order):
            apply_options(eng, ctx.defaults, ot.options)
            assert eng.plan(B, H, W)["structure"] == ot.structure, (ot.name, eng.plan_text(B, H, W))
            x = torch.from_numpy(synth.uniform_clips(B, ctx.tgt.T, H, W, seed=300 + i)).cuda()
            y = eng.forward(x)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(y).all()), ot.name
    finally:
        apply_options(eng, ctx.defaults, ctx.tgt.options)


def range_rerun(eng, ctx: Ctx) -> None:
    """History 4: conv0 x 4e5 (test_gpu_forward.test_split16_domain_activation_overflow_is_caught), a host-pointer forward - flagged,
    redone on the f32-MFMA kernels - under the library's default options, then the original weights and the target's options again."""
    from pfnl_amd import synth
    B, H, W = ctx.shape
    w = dict(ctx.weights)
    w["nlvsr/conv0/kernel"] = (w["nlvsr/conv0/kernel"] * 4e5).astype(np.float32)
    before = eng.range_reruns()
    apply_options(eng, ctx.defaults, ())
    try:
        eng.load_weights(w)
        y = eng.forward(synth.uniform_clips(B, ctx.tgt.T, H, W, seed=77))
        assert np.isfinite(y).all()
    finally:
        eng.load_weights(ctx.weights)
        apply_options(eng, ctx.defaults, ctx.tgt.options)
    assert eng.range_reruns() == before + 1, (before, eng.range_reruns())


def strip(eng, ctx: Ctx, kind: str = "nan") -> None:
    """History 5: forward_strip on the middle rows of a taller flood clip: Xo is written for the strip's queries only."""
    import torch
    B, H, W = ctx.shape
    Ht = 2 * H + FLOOD_DH
    x = flood_clip(kind, B, ctx.tgt.T, Ht, W)
    out = torch.zeros(eng.out_shape(B, Ht, W), dtype=torch.float32, device="cuda")
    r0 = (Ht // 3) & ~1
    eng.forward_strip(x, out, r0, (Ht // 3) & ~1)
    torch.cuda.synchronize()
    eng.range_flagged()
    s = eng.geom.scale
    assert not bool(torch.isfinite(out[:, :, s * r0:s * (r0 + 2)]).all()), "strip: the flood did not reach the output rows"
    del x, out


def session(eng, ctx: Ctx) -> None:
    """History 7: a streaming session at another raster, one batch of frames pushed, closed."""
    B, H, W = ctx.shape
    Hs, Ws = H + 6, W - 14
    rng = np.random.default_rng(H)
    with eng.open_stream(Hs, Ws, batch=2) as vs:
        got = []
        for _ in range(ctx.tgt.T // 2 + 2):      # the first window needs T // 2 frames ahead of it; two windows = one batch
            got += vs.push(rng.integers(0, 256, size=(Hs, Ws, 3), dtype=np.uint8))
        got += vs.pop_ready()
        got += vs.end()
        assert len(got) >= 2 and all(f.shape == (eng.geom.scale * Hs, eng.geom.scale * Ws, 3) for _, f in got)


# ---------------------------------------------------------------------------------------------------------------------------------
# the arena

PATTERN = {"float32": 0x7FC00000, "bfloat16": 0x7FC0, "int16": 0x7FFF}       # quiet NaN, quiet NaN, the largest int16
ITEMSIZE = {"float32": 4, "bfloat16": 2, "int16": 2}
ALIGN = 256


def _pattern_bytes(dtype: str, nbytes: int) -> np.ndarray:
    """nbytes (a multiple of 4) of the fill of `dtype`, little-endian."""
    unit = np.array([PATTERN[dtype]], dtype={4: "<u4", 2: "<u2"}[ITEMSIZE[dtype]]).view(np.uint8)
    return np.tile(unit, nbytes // unit.size)


@dataclass
class ArenaReport:
    changed: Optional[str]                       # None, or "gap byte N changed: K bytes after the end of `x`" style text of the FIRST change
    changed_bytes: int
    unwritten: Dict[str, int]                    # output operand -> elements still at their fill

    @property
    def ok(self) -> bool:
        return self.changed is None and not any(self.unwritten.values())

    def __str__(self) -> str:
        parts = []
        if self.changed:
            parts.append(f"{self.changed_bytes} gap bytes changed, the first: {self.changed}")
        parts += [f"{n} elements of `{k}` left at their fill" for k, n in self.unwritten.items() if n]
        return "; ".join(parts) or "arena untouched outside its operands, every output element written"


class Arena:
    """ONE allocation that holds the tensor operands of a call back to back: each 256-byte aligned, separated and surrounded by gaps of
    at least `gap_bytes` (one full frame of the call, so that a record count one tile - or one frame - too long still lands inside the
    arena), gaps and outputs filled with PATTERN.  operands: name -> (shape, dtype name, data or None); None marks an OUTPUT, which
    starts out at the fill.  `views[name]` are contiguous torch views of the allocation.  check() compares every gap AS INTEGERS (NaN
    does not equal NaN) with the fill and counts the output elements that still hold it."""

    def __init__(self, operands: Dict[str, tuple], gap_bytes: int, device="cuda"):
        import torch
        tdt = {"float32": torch.float32, "bfloat16": torch.bfloat16, "int16": torch.int16}
        gap = (int(gap_bytes) + ALIGN - 1) // ALIGN * ALIGN
        self.gap_bytes = gap
        self.spans: List[Tuple[str, int, int, str, bool]] = []       # (name, begin, end, dtype, is_output), bytes from the aligned base
        off = gap
        for name, (shape, dtype, data) in operands.items():
            n = int(np.prod(shape)) * ITEMSIZE[dtype]
            assert n > 0 and n % 4 == 0, (name, shape, dtype)         # (the fills keep their phase: every span begins and ends on a 4-byte boundary)
            self.spans.append((name, off, off + n, dtype, data is None))
            off = (off + n + ALIGN - 1) // ALIGN * ALIGN + gap
        self.nbytes = off
        self.buf = torch.empty(self.nbytes + ALIGN, dtype=torch.uint8, device=device)
        self.base = (-self.buf.data_ptr()) % ALIGN
        # the image of the arena before the call: fills everywhere (a gap: first half the operand's in front of it, second half the one's
        # behind it, so that a read past either end meets that operand's own NaN), then the inputs' data
        img = np.empty(self.nbytes, np.uint8)
        prev_end, prev_dt = 0, self.spans[0][3]
        for name, b, e, dtype, _ in self.spans + [("", self.nbytes, self.nbytes, self.spans[-1][3], False)]:
            mid = (prev_end + (b - prev_end) // 2) // 4 * 4
            img[prev_end:mid] = _pattern_bytes(prev_dt, mid - prev_end + 3)[:mid - prev_end]
            img[mid:b] = _pattern_bytes(dtype, b - mid + 3)[:b - mid]
            if e > b:
                img[b:e] = _pattern_bytes(dtype, e - b + 3)[:e - b]
            prev_end, prev_dt = e, dtype
        self.gap_mask = np.ones(self.nbytes, bool)
        for name, b, e, dtype, _ in self.spans:
            self.gap_mask[b:e] = False
            data = operands[name][2]
            if data is not None:
                t = data if isinstance(data, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(data))
                img[b:e] = t.detach().cpu().contiguous().view(torch.uint8).reshape(-1).numpy()
        self.image = img
        self.buf[self.base:self.base + self.nbytes] = torch.from_numpy(img).to(device)
        self.views = {}
        for name, b, e, dtype, _ in self.spans:
            v = self.buf[self.base + b:self.base + e].view(tdt[dtype]).view(*operands[name][0])
            assert v.is_contiguous() and v.data_ptr() % ALIGN == 0
            self.views[name] = v

    def __getitem__(self, name):
        return self.views[name]

    def locate(self, off: int) -> str:
        """A gap byte's place relative to the nearest operand."""
        best = None
        for name, b, e, _, _ in self.spans:
            for d, text in ((off - e, f"{off - e} bytes past the end of `{name}`"), (b - 1 - off, f"{b - off} bytes before `{name}`")):
                if d >= 0 and (best is None or d < best[0]):
                    best = (d, text)
        return best[1]

    def check(self) -> ArenaReport:
        now = self.buf[self.base:self.base + self.nbytes].cpu().numpy()
        diff = (now != self.image) & self.gap_mask
        changed, nchanged = None, int(diff.sum())
        if nchanged:
            first = int(np.argmax(diff))
            changed = f"byte {first} of the arena, {self.locate(first)}: 0x{int(now[first]):02x} where the fill has 0x{int(self.image[first]):02x}"
        unwritten = {}
        for name, b, e, dtype, is_out in self.spans:
            if is_out:
                w = {4: "<u4", 2: "<u2"}[ITEMSIZE[dtype]]
                unwritten[name] = int((now[b:e].view(w) == PATTERN[dtype]).sum())
        return ArenaReport(changed, nchanged, unwritten)
