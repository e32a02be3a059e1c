"""The kernels on tensors past 2^31 and 2^32 bytes (and past 2^31 elements, and past 65535 items), on a real MI355X.

The reference harness works in `part`-sized batches: at UDM10 one 64-channel fp32 activation of a batch is 3.3 GB.  Two conventions keep such
batches right - every trunk kernel reaches ONE item through a buffer resource with 32-bit offsets placed at ptr + (size_t)item * H * W * 64,
every flat kernel walks a size_t total - and a dropped cast in either breaks nothing at the sizes of the other test files.  Here frames stay
tiny and items are many (tests/big.py), so that a 32-bit wrap sends an item to another item's address inside the same tensor.

Each case: inputs drawn on the device from a seeded generator; the output handed over full of NaN and checked for NaN afterwards; the items
at the thresholds, the first and the last against the hook's fp64 spec at the hook's own tolerance (imported from test_gpu_ops.py /
test_gpu_bf16.py); the WHOLE output against the same hook run over slices of whole chains, each below 2^31 bytes, at twice that tolerance
(both sides lie within one tolerance of fp64), which finds an item written in another item's place; the inputs' checksums before and after.
The parts comparison is BIT EQUALITY where the launcher gives every item its own workgroups or threads with a fixed order of work, whatever
the batch (each such test says where that is read); it is the bound for the persistent launches (which chains a workgroup takes follows
the chain count), the split-chain cuts and the non-local kernels (the key split follows B).
The copy and flat kernels compare the whole tensor with the torch expression of their rule, bit for bit."""
import gc
import math
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

import big  # noqa: E402
import test_gpu_bf16 as TB  # noqa: E402   (close_bf16, ref_conv3, _base_ref, ACCUM_BF16_REL_TOL)
import test_gpu_ops as TO  # noqa: E402    (the hooks' tolerances against the fp64 spec, _grid)
from oracle import pfnl_spec  # noqa: E402
from pfnl_amd import _capi, ops, synth  # noqa: E402

H0, W0 = big.DEFAULT_HW            # 33 x 70
HE, WE = 34, 70                    # the Winograd kernels need even H, W
T = big.T
CHUNK = 1 << 27                    # elements per piece of the device-side reductions

_SKIPPED = []                      # cases that found too little free memory
TIMES = {}                         # case -> (seconds of the big call, footprint in bytes); printed by the last test


# ---- device-side helpers -----------------------------------------------------------------------------------------------------------------
def _reserve(name, need):
    """Skip unless 1.25 x the case's footprint is free; the skip names both numbers."""
    assert need <= big.MAX_CASE_BYTES, (name, need)
    free, _ = torch.cuda.mem_get_info()
    if free < 1.25 * need:
        _SKIPPED.append(name)
        pytest.skip(f"{name}: needs 1.25 x {need} = {int(1.25 * need)} bytes of device memory, {free} bytes are free")


@pytest.fixture(autouse=True)
def _release():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _gen(seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return g


def _draw(shape, dtype, g, kind="normal", scale=1.0):
    """A tensor of ``shape`` drawn piecewise on the device (no host array, no fp32 copy of a whole bf16 tensor)."""
    t = torch.empty(shape, dtype=dtype, device="cuda")
    flat = t.view(-1)
    for i in range(0, flat.numel(), CHUNK):
        m = min(CHUNK, flat.numel() - i)
        if kind == "normal":
            p = torch.randn(m, generator=g, device="cuda", dtype=torch.float32)
        else:
            p = torch.rand(m, generator=g, device="cuda", dtype=torch.float32)
        if scale != 1.0:
            p *= scale
        flat[i:i + m] = p
    return t


def _nan(shape, dtype=torch.float32):
    return torch.full(tuple(shape), float("nan"), dtype=dtype, device="cuda")


def _has_nan(t):
    flat = t.reshape(-1) if t.is_contiguous() else None
    if flat is None:
        return bool(torch.isnan(t).any())
    return any(bool(torch.isnan(flat[i:i + CHUNK]).any()) for i in range(0, flat.numel(), CHUNK))


def _all_nan(t):
    flat = t.view(-1)
    return all(bool(torch.isnan(flat[i:i + CHUNK]).all()) for i in range(0, flat.numel(), CHUNK))


def _checksum(t):
    """(sum, position-weighted sum) of the tensor's bit patterns, exact in int64 arithmetic modulo 2^64."""
    flat = t.view(-1).view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
    s = w = 0
    for i in range(0, flat.numel(), CHUNK):
        p = flat[i:i + CHUNK].to(torch.int64)
        s += int(p.sum())
        w += int((p * (torch.arange(p.numel(), device="cuda", dtype=torch.int64) % 8191 + 1)).sum())
        w = (w + i) & ((1 << 64) - 1)
    return s, w


def _nbytes(rows, tail, dtype):
    return rows * math.prod(tail) * torch.empty((), dtype=dtype).element_size()


# ---- the comparisons: one rule per kind, for the selected items against the spec (host) and for the parts run (device, twice the bound) -----
def _close_spec(kind, tol, got, ref, what):
    """``got`` (a CPU tensor of one unit) against ``ref`` at the hook's own tolerance."""
    if kind == "bf16":
        TB.close_bf16(got, ref.float())
        return
    if kind == "bits":
        assert torch.equal(got, ref), what
        return
    g, r = got.double(), ref.double()
    e = float((g - r).abs().max())
    if kind == "relmax":
        assert e < tol * max(1.0, float(r.abs().max())), (what, e)
    elif kind == "abs":
        assert e < tol, (what, e)
    elif kind == "relstep":
        rel = float(((g - r).abs() / r.abs().clamp_min(2.0 ** -14)).max())
        assert rel <= tol, (what, rel)
    else:
        raise KeyError(kind)


def _close_parts(kind, tol, whole, part, what):
    """A slice of the big call's output against the same hook run on that slice alone, on the device: twice the hook's tolerance."""
    if kind == "bits":
        assert torch.equal(whole, part), what
        return
    w, p = whole.float(), part.float()
    d = (w - p).abs_()
    if kind == "bf16":
        bound = p.abs_().mul_(2.0 ** -7).add_(1e-5).mul_(2.0)
        assert bool((d <= bound).all()), (what, float((d - bound).max()))
    elif kind == "relmax":
        e, s = float(d.max()), max(1.0, float(p.abs_().max()))
        assert e < 2.0 * tol * s, (what, e, s)
    elif kind == "abs":
        e = float(d.max())
        assert e < 2.0 * tol, (what, e)
    elif kind == "relstep":
        rel = float((d / p.abs_().clamp_min_(2.0 ** -14)).max())
        assert rel <= 2.0 * tol, (what, rel)
    else:
        raise KeyError(kind)


# ---- the runner ------------------------------------------------------------------------------------------------------------------------------
class Case:
    """One hook over ``units`` units (chains / clips / items).  ins / outs: name -> (rows per unit, shape of a row, dtype[, draw kind, scale]);
    call(I, O, units) runs the hook on tensors of any whole number of units; spec(I1) -> name -> the reference of ONE unit (CPU tensors
    in, CPU tensors out); tol: name -> (kind, tolerance); staging(units) -> bytes the hook allocates beside its arguments."""

    def __init__(self, name, units, ins, outs, call, spec, tol, staging=None, seed=1, parts_bits=False):
        self.name, self.units, self.ins, self.outs, self.call, self.spec, self.tol = name, units, ins, outs, call, spec, tol
        self.staging = staging or (lambda u: 0)
        self.seed = seed
        self.parts_bits = parts_bits        # the per-item work order cannot depend on the batch: the parts run must give the same bits
        self.spec_sees_outputs = False      # spec(I1, O1): the reference of one output is stated on another output of the same call


def _selected_units(c):
    sel = {0, c.units - 1}
    for rows, tail, dtype, *_ in list(c.ins.values()) + list(c.outs.values()):
        rb = _nbytes(1, tail, dtype)
        for i in big.selected_items(rb, 1, 1, rows * c.units):
            sel.add(i // rows)
    return sorted(sel)


def run_case(c):
    tensors = list(c.ins.items()) + list(c.outs.items())
    unit_bytes = {k: _nbytes(v[0], v[1], v[2]) for k, v in tensors}
    sl = big.slices(c.units, max(unit_bytes.values()))
    pmax = max(u1 - u0 for u0, u1 in sl)
    out_unit = sum(unit_bytes[k] for k in c.outs)
    need = big.footprint([unit_bytes[k] * c.units for k, _ in tensors], staging=c.staging(c.units),
                         parts_bytes=pmax * out_unit + 6 * pmax * max(unit_bytes[k] for k in c.outs))
    _reserve(c.name, need)
    assert any(big.crosses(unit_bytes[k], 1, 1, c.units, big.TIER_B) for k, _ in tensors), "no tensor of the case crosses 2^32 bytes"
    g = _gen(c.seed)
    I = {k: _draw((v[0] * c.units,) + tuple(v[1]), v[2], g, *(v[3:] or ("normal", 1.0))) for k, v in c.ins.items()}
    before = {k: _checksum(t) for k, t in I.items()}
    O = {k: _nan((v[0] * c.units,) + tuple(v[1]), v[2]) for k, v in c.outs.items()}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    c.call(I, O, c.units)
    torch.cuda.synchronize()
    TIMES[c.name] = (time.perf_counter() - t0, need)
    for k, t in O.items():
        assert not _has_nan(t), f"{c.name}: {k} keeps NaN - not every element was written"
    assert {k: _checksum(t) for k, t in I.items()} == before, f"{c.name}: the call changed its inputs"
    # the items at the thresholds, the first and the last, against the spec
    for u in _selected_units(c):
        I1 = {k: t[u * c.ins[k][0]:(u + 1) * c.ins[k][0]].cpu() for k, t in I.items()}
        O1 = {k: t[u * c.outs[k][0]:(u + 1) * c.outs[k][0]].cpu() for k, t in O.items()}
        R = c.spec(I1, O1) if c.spec_sees_outputs else c.spec(I1)
        for k, ref in R.items():
            kind, tol = c.tol[k]
            _close_spec(kind, tol, O1[k], ref, (c.name, k, "unit", u))
    # the whole tensor against the hook over slices of whole units, each below 2^31 bytes
    P = {k: _nan((v[0] * pmax,) + tuple(v[1]), v[2]) for k, v in c.outs.items()}
    for u0, u1 in sl:
        n = u1 - u0
        for t in P.values():
            t.fill_(float("nan"))
        c.call({k: t[u0 * c.ins[k][0]:u1 * c.ins[k][0]] for k, t in I.items()}, {k: t[:n * c.outs[k][0]] for k, t in P.items()}, n)
        for k, t in O.items():
            r = c.outs[k][0]
            kind, tol = c.tol[k]
            whole, part = t[u0 * r:u1 * r], P[k][:n * r]
            _close_parts("bits" if c.parts_bits else kind, tol, whole, part, (c.name, k, "units", u0, u1))


# ---- host weights and fp64 specs ---------------------------------------------------------------------------------------------------------------
def _w(seed, shape, div):
    return (np.random.default_rng(seed).normal(size=shape) / div).astype(np.float32)


def _bias(seed, n=64):
    return (np.random.default_rng(seed + 99).normal(size=n) * 0.1).astype(np.float32)


def _f64(t):
    return t.numpy().astype(np.float64)


def _conv64(x, k, b):
    return pfnl_spec.conv2d_same(x, k.astype(np.float64), None if b is None else b.astype(np.float64))


def _cat_frames(x64, n, Tn):
    _, H, W, Cc = x64.shape
    return x64.reshape(n, Tn, H, W, Cc).transpose(0, 2, 3, 1, 4).reshape(n, H, W, Tn * Cc)


def _units_fp32(H, W):
    return big.items_for(256, H, W, T, big.TIER_B) // T


def _x_bytes(units, H, W, bpp=256):
    return units * T * H * W * bpp


def _split_units(units, H, W):
    """The plan's rule (test_gpu_ops._split_case) at this chain count: the smallest count of clips >= ``units`` whose chains leave a partial
    last round of R chains with 3 R <= grid, cut frame by frame (T = 3: split_s = 3, split_q = 1)."""
    G = TO._grid()
    for u in range(units, units + G + 1):
        nch = TO._chains(u, H, W)
        R = nch % G
        if 0 < 3 * R <= G:
            return u, (nch - R, 3, 1)
    raise AssertionError("no split geometry near this chain count")


# ---- tier B: the fp32 trunk ------------------------------------------------------------------------------------------------------------------------
def _fused3x3_case(name, call, tol, H, W, staging=0.0):
    units = _units_fp32(H, W)
    k, b = _w(1, (3, 3, 64, 64), 24.0), _bias(1)
    row = (H, W, 64)

    def spec(I1):
        y = _conv64(_f64(I1["x"]), k, b) + np.repeat(_f64(I1["addend"]), T, axis=0)
        return {"out": torch.from_numpy(pfnl_spec.lrelu(y) + _f64(I1["resid"]))}

    return Case(name, units, {"x": (T, row, torch.float32), "addend": (1, row, torch.float32), "resid": (T, row, torch.float32)},
                {"out": (T, row, torch.float32)}, lambda I, O, n: call(I["x"], k, b, I["addend"], I["resid"], O["out"]), spec,
                {"out": ("relmax", tol)}, staging=lambda u: int(staging * _x_bytes(u, H, W)))


@pytest.mark.parametrize("variant", ["split16", "split16_sf_in", "winograd", "winograd_ws"])
def test_conv3x3_fused_past_4g(variant):
    """conv3x3_winograd(variant=...) with addend / add_div = 3 / resid on 7266 items (7053 of 34 x 70 for the Winograd kernels, which need
    even sizes): conv3x3_split16_kernel, conv3x3_sf_kernel, conv_wino_kernel, conv_wino_ws_kernel."""
    wino = variant.startswith("winograd")
    H, W = (HE, WE) if wino else (H0, W0)
    tol = TO.WINOGRAD_REL_TOL if wino else TO.SPLIT16_OP_REL_TOL
    run_case(_fused3x3_case(f"conv3x3_winograd[{variant}]", lambda x, k, b, a, r, o: ops.conv3x3_winograd(
        x, k, b, act=True, addend=a, add_div=T, resid=r, variant=variant, out=o), tol, H, W, staging=0.5 if variant == "split16_sf_in" else 0.0))


def test_conv2d_fused_past_4g():
    """conv2d (conv_mfma.hip: the item rides in blockIdx.z, 7266 of them) with the fused conv2 epilogue.  The parts run must give the same
    bits: launch_conv_mfma takes the one fused instantiation <3, 16, 2, true> whatever the batch, launch_variant's grid is (tiles across,
    tiles down, items), and a workgroup walks its tile's K chunks in a fixed order."""
    c = _fused3x3_case("conv2d", lambda x, k, b, a, r, o: ops.conv2d(x, k, b, act=True, addend=a, add_div=T, resid=r, out=o),
                       TO.F32_MFMA_REL_TOL, H0, W0)
    c.parts_bits = True
    run_case(c)


def test_conv3x3_split16_sf_out_past_4g():
    """conv1_i writing the split format (variant split16_sf_out: conv3x3_split16_kernel<0, OSF>, the hook converts back to fp32).  Its test
    in test_gpu_ops.py holds it to the fp32-output launch of the same kernel (variant split16) at 2^-21 per element, and that launch to the
    fp64 spec at SPLIT16_OP_REL_TOL; the bound against fp64 here is the sum of the two (|v| <= max|spec|), by the triangle inequality.
    No addend / resid: the hook has no fused form of this variant (pfnl_op_conv3x3_split16_sf refuses an addend unless which = 0 or 2)."""
    units = _units_fp32(H0, W0)
    k, b = _w(2, (3, 3, 64, 64), 24.0), _bias(2)
    row = (H0, W0, 64)
    spec = lambda I1: {"out": torch.from_numpy(pfnl_spec.lrelu(_conv64(_f64(I1["x"]), k, b)))}  # noqa: E731
    run_case(Case("conv3x3_winograd[split16_sf_out]", units, {"x": (T, row, torch.float32)}, {"out": (T, row, torch.float32)},
                  lambda I, O, n: ops.conv3x3_winograd(I["x"], k, b, act=True, variant="split16_sf_out", out=O["out"]), spec,
                  {"out": ("relmax", TO.SPLIT16_OP_REL_TOL + TO.SF_OUT_REL_STEP)}, staging=lambda u: _x_bytes(u, H0, W0) // 2))


def _chain_case(name, call, units, H=H0, W=W0):
    k2, b = _w(3, (3, 3, 128, 64), 34.0), _bias(3)
    row = (H, W, 64)

    def spec(I1):
        cat = np.concatenate([np.repeat(_f64(I1["base"]), T, axis=0), _f64(I1["x"])], axis=-1)
        return {"out": torch.from_numpy(pfnl_spec.lrelu(_conv64(cat, k2, b)) + _f64(I1["resid"]))}

    return Case(name, units, {"x": (T, row, torch.float32), "base": (1, row, torch.float32), "resid": (T, row, torch.float32)},
                {"out": (T, row, torch.float32)}, lambda I, O, n: call(I["x"], k2, b, I["base"], I["resid"], O["out"], n), spec,
                {"out": ("relmax", TO.SPLIT16_OP_REL_TOL)}, staging=lambda u: _x_bytes(u, H, W) * 2 // 3)


@pytest.mark.parametrize("form", ["sf_chain", "mfma32", "mfma16", "split"])
def test_conv2_chain_past_4g(form):
    """The whole of conv2_i in one launch: variant split16_sf_chain, conv2_chain_ex with both MFMA shapes, and conv2_chain_ex cut by the
    plan's rule at this chain count (conv3x3_sf_chain_kernel<false, true>: the cut chains' parts index `partial` at these sizes)."""
    units = _units_fp32(H0, W0)
    if form == "sf_chain":
        call = lambda x, k, b, ba, r, o, n: ops.conv3x3_winograd(x, k, b, act=True, addend=ba, add_div=T, resid=r, variant="split16_sf_chain", out=o)  # noqa: E731
    elif form == "split":
        units, split = _split_units(units, H0, W0)
        G = TO._grid()

        def call(x, k, b, ba, r, o, n):                                    # a slice has its own chain count: the same rule there
            nch = TO._chains(n, H0, W0)
            R = nch % G
            ops.conv2_chain_ex(x, k, b, ba, r, T, split=(nch - R, 3, 1) if 0 < 3 * R <= G else (0, 0, 0), out=o)
    else:
        call = lambda x, k, b, ba, r, o, n: ops.conv2_chain_ex(x, k, b, ba, r, T, mfma=int(form[4:]), out=o)  # noqa: E731
    run_case(_chain_case(f"conv2_chain[{form}]", call, units))


def _c1c10_case(name, call, units, H=H0, W=W0):
    k1, b1, k10, b10 = _w(4, (3, 3, 64, 64), 24.0), _bias(4), _w(5, (1, 1, 64 * T, 64), math.sqrt(64 * T)), _bias(5)
    row = (H, W, 64)

    def spec(I1):
        r1 = pfnl_spec.lrelu(_conv64(_f64(I1["x"]), k1, b1))
        rb = pfnl_spec.lrelu(_conv64(_cat_frames(r1, 1, T), k10, b10))
        return {"out1": torch.from_numpy(r1), "base": torch.from_numpy(rb)}

    return Case(name, units, {"x": (T, row, torch.float32)}, {"out1": (T, row, torch.float32), "base": (1, row, torch.float32)},
                lambda I, O, n: call(I["x"], k1, b1, k10, b10, O["out1"], O["base"], n), spec,
                {"out1": ("relmax", TO.SPLIT16_OP_REL_TOL), "base": ("relmax", TO.SPLIT16_OP_REL_TOL)},
                staging=lambda u: _x_bytes(u, H, W) * 2 // 3 + (1 << 28))


@pytest.mark.parametrize("form", ["plain", "mfma32", "mfma16", "split"])
def test_conv1_conv10_split16_past_4g(form):
    """conv1_i + conv10_i in one launch (conv3x3_c1c10_kernel): conv1_conv10_split16, conv1_conv10_split16_mfma in both MFMA shapes, and
    conv1_conv10_split16_ex cut by the plan's rule at this chain count (c10_finalize_kernel and `partial` at these sizes)."""
    units = _units_fp32(H0, W0)
    if form == "plain":
        call = lambda x, k1, b1, k10, b10, o1, ob, n: ops.conv1_conv10_split16(x, k1, b1, k10, b10, T, out1=o1, base=ob)  # noqa: E731
    elif form == "split":
        units, _ = _split_units(units, H0, W0)
        G = TO._grid()

        def call(x, k1, b1, k10, b10, o1, ob, n):
            nch = TO._chains(n, H0, W0)
            R = nch % G
            ops.conv1_conv10_split16_ex(x, k1, b1, k10, b10, T, split=(nch - R, 3, 1) if 0 < 3 * R <= G else (0, 0, 0), out1=o1, base=ob)
    else:
        call = lambda x, k1, b1, k10, b10, o1, ob, n: ops.conv1_conv10_split16_mfma(x, k1, b1, k10, b10, T, mfma=int(form[4:]), out1=o1, base=ob)  # noqa: E731
    run_case(_c1c10_case(f"conv1_conv10_split16[{form}]", call, units))


@pytest.mark.parametrize("form", ["winograd", "split16", "split16_ex", "split"])
def test_conv3x3_accum_past_4g(form):
    """convmerge1 at cout = 48 over 3 frames: conv3x3_accum in both variants, conv3x3_accum_split16_ex whole and cut by the plan's rule.  The
    hooks' buffer has 64 channels; the result is its first 48, and those are what is checked for NaN and compared."""
    H, W = (HE, WE) if form == "winograd" else (H0, W0)
    units = _units_fp32(H, W)
    cout = 48
    k, b = _w(6, (3, 3, 64 * T, cout), math.sqrt(576 * T)), _bias(6, cout)
    G = TO._grid()
    if form == "split":
        units, _ = _split_units(units, H, W)

    def call(I, O, n):
        O["out"][..., cout:] = 0.0                                       # outside the result: the same on both sides of every comparison
        if form in ("winograd", "split16"):
            ops.conv3x3_accum(I["x"], k, b, act=True, frames_per_clip=T, variant=form, out=O["out"])
            return
        nch = TO._chains(n, H, W)
        R = nch % G
        split = (nch - R, 3, 1) if form == "split" and 0 < 3 * R <= G else (0, 0, 0)
        ops.conv3x3_accum_split16_ex(I["x"], k, b, act=True, frames_per_clip=T, split=split, out=O["out"])

    def spec(I1):
        r = pfnl_spec.lrelu(_conv64(_cat_frames(_f64(I1["x"]), 1, T), k, b))
        return {"out": F.pad(torch.from_numpy(r), (0, 64 - cout))}

    tol = TO.WINOGRAD_REL_TOL if form in ("winograd", "split16") else TO.SPLIT16_OP_REL_TOL
    run_case(Case(f"conv3x3_accum[{form}]", units, {"x": (T, (H, W, 64), torch.float32)}, {"out": (1, (H, W, 64), torch.float32)}, call,
                  spec, {"out": ("relmax", tol)}, staging=lambda u: 1 << 28))


@pytest.mark.parametrize("variant", ["stream", "split16", "split16_sf:10", "split16_sf:01", "split16_sf:11"])
def test_conv1x1_stream_past_4g(variant):
    """conv10_i over 3 frames: conv1x1_stream_kernel, the split-f16 kernel at the fp32 interface and in the three split-format forms.
    Variant stream must give the same bits in parts: launch_conv1x1_stream has one form, a wave owns one group of 32 pixels of one item
    (ngroups = ceil(HW / 32) * items) and walks the T frames in order.  (launch_conv1x1_split16 picks 2 or 8 waves a workgroup by the
    group count: the bound.)"""
    units = _units_fp32(H0, W0)
    k, b = _w(7, (1, 1, 64 * T, 64), math.sqrt(64 * T)), _bias(7)
    spec = lambda I1: {"out": torch.from_numpy(pfnl_spec.lrelu(_conv64(_cat_frames(_f64(I1["x"]), 1, T), k, b)))}  # noqa: E731
    tol = TO.SPLIT16_OP_REL_TOL if "sf" in variant else TO.F32_MFMA_REL_TOL
    run_case(Case(f"conv1x1_stream[{variant}]", units, {"x": (T, (H0, W0, 64), torch.float32)}, {"out": (1, (H0, W0, 64), torch.float32)},
                  lambda I, O, n: ops.conv1x1_stream(I["x"], k, b, act=True, frames_per_item=T, variant=variant, out=O["out"]), spec,
                  {"out": ("relmax", tol)}, staging=lambda u: _x_bytes(u, H0, W0) * 2 // 3 if "sf" in variant else 0,
                  parts_bits=variant == "stream"))


def test_conv2_grouped_past_4g():
    """conv2_i on the persistent Winograd kernel with the shared base (34 x 70: even sizes)."""
    c = _chain_case("conv2_grouped", lambda x, k, b, ba, r, o, n: ops.conv2_grouped(x, ba, k, b, r, T, out=o), _units_fp32(HE, WE), HE, WE)
    c.tol = {"out": ("relmax", TO.WINOGRAD_REL_TOL)}
    c.staging = lambda u: 0
    run_case(c)


def test_conv_small_past_4g():
    """conv_small.hip in its conv2_i form: a = base (a_div = 3), b = inp1, + resid."""
    c = _chain_case("conv_small", lambda x, k, b, ba, r, o, n: ops.conv_small(x, k, b, a=ba, a_div=T, resid=r, out=o), _units_fp32(H0, W0))
    c.staging = lambda u: 0
    run_case(c)


def test_conv_small_pf_block_past_4g():
    """One progressive-fusion block on the small-shape kernels, two launches; the per-frame partials are a fourth tensor past 2^32 bytes."""
    units = _units_fp32(H0, W0)
    k1, b1, k10, b10 = _w(8, (3, 3, 64, 64), 24.0), _bias(8), _w(9, (1, 1, 64 * T, 64), math.sqrt(64 * T)), _bias(9)
    k2, b2 = _w(10, (3, 3, 128, 64), 34.0), _bias(10)
    row = (H0, W0, 64)

    def spec(I1):
        x64 = _f64(I1["x"])
        r1 = pfnl_spec.lrelu(_conv64(x64, k1, b1))
        rb = pfnl_spec.lrelu(_conv64(_cat_frames(r1, 1, T), k10, b10))
        r2 = x64 + pfnl_spec.lrelu(_conv64(np.concatenate([np.repeat(rb, T, axis=0), r1], axis=-1), k2, b2))
        return {"inp1": torch.from_numpy(r1), "out": torch.from_numpy(r2)}

    run_case(Case("conv_small_pf_block", units, {"x": (T, row, torch.float32)}, {"inp1": (T, row, torch.float32), "out": (T, row, torch.float32)},
                  lambda I, O, n: ops.conv_small_pf_block(I["x"], k1, b1, k10, b10, k2, b2, T, inp1=O["inp1"], out=O["out"]), spec,
                  {"inp1": ("relmax", TO.SPLIT16_OP_REL_TOL), "out": ("relmax", TO.SMALL_BLOCK_OUT_REL_TOL)},
                  staging=lambda u: _x_bytes(u, H0, W0)))


# ---- tier A where it is another path: a frame the 32-bit offsets of the persistent kernels cannot address is refused on the host ------------------
@pytest.mark.parametrize("hook", ["conv3x3_accum[winograd]", "conv3x3_accum[split16]", "conv2_grouped"])
def test_one_frame_past_2g_bytes_is_refused_before_any_launch(hook):
    """One frame of 2896 x 2898 x 64 fp32 is 0x800fa000 bytes: past the out-of-range offset 0x7fffffff of a per-item buffer resource.  The
    hooks of the persistent kernels check it first thing (frame_too_large in pfnl_op_conv3x3_accum, pfnl_op_conv3x3_accum_split16 and
    pfnl_op_conv2_grouped, capi_ops.hip: before the weight pack, any allocation and any launch), so the call raises and the NaN-filled
    output is untouched.  (The forward's plan sends such frames to the per-tile kernels: launch_plan.h fits32.)"""
    Hh, Ww = 2896, 2898
    one = Hh * Ww * 256
    assert one > big.TIER_A - 1
    n = 4 if hook == "conv2_grouped" else 2
    _reserve(hook, big.footprint([one] * n))
    x = _draw((1, Hh, Ww, 64), torch.float32, _gen(95))
    out = _nan((1, Hh, Ww, 64))
    with pytest.raises(_capi.PFNLHipError, match="frame too large"):
        if hook == "conv2_grouped":
            ops.conv2_grouped(x, x, _w(1, (3, 3, 128, 64), 34.0), _bias(1), x, 1, out=out)
        else:
            ops.conv3x3_accum(x, _w(1, (3, 3, 64, 48), 24.0), _bias(1, 48), frames_per_clip=1, variant=hook[14:-1], out=out)
    torch.cuda.synchronize()
    assert _all_nan(out)


# ---- tier E: fp32 tensors past 2^31 ELEMENTS (8.6 GB), where an `int` item * H * W * 64 wraps; the one-input hooks -------------------------------
@pytest.mark.parametrize("hook", ["conv3x3_split16", "conv2d", "conv1x1_split16", "conv1x1_stream", "conv3x3_accum_split16"])
def test_fp32_trunk_past_2g_elements(hook):
    """At tier B an fp32 tensor holds 2^30 elements, so only 32-bit BYTE arithmetic wraps there.  14 529 items of 33 x 70 x 64 fp32 carry the
    input past element 2^31: the plain 3x3 launches of conv_split16.hip and conv_mfma.hip (output as large), both conv10_i kernels and
    convmerge1 on the split-f16 kernel (one output item per 3 input items).  conv2d and conv1x1_stream must give the same bits in parts:
    every slice has far more than the 768 tiles at which launch_conv_mfma changes the tile height, so all runs take <3, 16, 2, false> with
    the item in blockIdx.z; conv1x1_stream as in test_conv1x1_stream_past_4g."""
    units = big.items_for(256, H0, W0, T, big.TIER_E) // T
    row = (H0, W0, 64)
    if hook in ("conv3x3_split16", "conv2d"):
        k, b = _w(31, (3, 3, 64, 64), 24.0), _bias(31)
        spec = lambda I1: {"out": torch.from_numpy(pfnl_spec.lrelu(_conv64(_f64(I1["x"]), k, b)))}  # noqa: E731
        if hook == "conv2d":
            call, tol = (lambda I, O, n: ops.conv2d(I["x"], k, b, act=True, out=O["out"])), TO.F32_MFMA_REL_TOL
        else:
            call, tol = (lambda I, O, n: ops.conv3x3_winograd(I["x"], k, b, act=True, variant="split16", out=O["out"])), TO.SPLIT16_OP_REL_TOL
        rows_out = T
    elif hook.startswith("conv1x1"):
        k, b = _w(32, (1, 1, 64 * T, 64), math.sqrt(64 * T)), _bias(32)
        spec = lambda I1: {"out": torch.from_numpy(pfnl_spec.lrelu(_conv64(_cat_frames(_f64(I1["x"]), 1, T), k, b)))}  # noqa: E731
        variant = hook[8:]
        call, tol, rows_out = (lambda I, O, n: ops.conv1x1_stream(I["x"], k, b, act=True, frames_per_item=T, variant=variant, out=O["out"])), TO.F32_MFMA_REL_TOL, 1
    else:
        k, b = _w(33, (3, 3, 64 * T, 64), math.sqrt(576 * T)), _bias(33)
        spec = lambda I1: {"out": torch.from_numpy(pfnl_spec.lrelu(_conv64(_cat_frames(_f64(I1["x"]), 1, T), k, b)))}  # noqa: E731
        call, tol, rows_out = (lambda I, O, n: ops.conv3x3_accum_split16_ex(I["x"], k, b, act=True, frames_per_clip=T, out=O["out"])), TO.SPLIT16_OP_REL_TOL, 1
    c = Case(f"past 2^31 elements[{hook}]", units, {"x": (T, row, torch.float32)}, {"out": (rows_out, row, torch.float32)}, call, spec,
             {"out": ("relmax", tol)}, staging=lambda u: 1 << 28, parts_bits=hook in ("conv2d", "conv1x1_stream"))
    assert big.crosses(_nbytes(T, row, torch.float32), 1, 1, units, big.TIER_E)
    run_case(c)


# ---- tier B: the bf16 trunk (128 bytes per pixel: twice the items) ---------------------------------------------------------------------------------
BF16_UNITS = 2 * _units_fp32(H0, W0)                                    # 4844 chains = 14 532 items
ROW16 = (H0, W0, 64)


def _bf16_fused_case(name, call, units=BF16_UNITS):
    k, b = _w(11, (3, 3, 64, 64), 20.0), _bias(11)
    spec = lambda I1: {"out": TB.ref_conv3(I1["x"].float(), k, b, True, I1["addend"].float(), T, I1["resid"].float())}  # noqa: E731
    bf = torch.bfloat16
    return Case(name, units, {"x": (T, ROW16, bf), "addend": (1, ROW16, bf), "resid": (T, ROW16, bf)}, {"out": (T, ROW16, bf)},
                lambda I, O, n: call(I["x"], k, b, I["addend"], I["resid"], O["out"], n), spec, {"out": ("bf16", None)})


@pytest.mark.parametrize("form", ["plain", "mfma32", "mfma16", "split"])
def test_conv3x3_bf16_past_4g(form):
    """The fused bf16 3x3 kernel on 14 532 items: conv3x3_bf16, conv3x3_bf16_ex in both MFMA shapes and with the plan's cut."""
    G = TO._grid()
    units = BF16_UNITS
    if form == "plain":
        call = lambda x, k, b, a, r, o, n: ops.conv3x3_bf16(x, k, b, act=True, addend=a, add_div=T, resid=r, out=o)  # noqa: E731
    elif form == "split":
        units, _ = _split_units(units, H0, W0)

        def call(x, k, b, a, r, o, n):
            nch = TO._chains(n, H0, W0)
            R = nch % G
            ops.conv3x3_bf16_ex(x, k, b, a, T, r, split=(nch - R, 3, 1) if 0 < 3 * R <= G else (0, 0, 0), out=o)
    else:
        call = lambda x, k, b, a, r, o, n: ops.conv3x3_bf16_ex(x, k, b, a, T, r, mfma=int(form[4:]), out=o)  # noqa: E731
    run_case(_bf16_fused_case(f"conv3x3_bf16[{form}]", call, units))


@pytest.mark.parametrize("form", ["plain", "mfma32", "mfma16", "split"])
def test_conv1_conv10_bf16_past_4g(form):
    """conv1_i + conv10_i in one launch of the bf16 kernel, and its _ex form in both MFMA shapes and cut (c10_finalize_bf16 at these sizes).
    `base` is held to the 1x1 of the kernel's own, already rounded, out1, as in test_conv1_conv10_bf16_one_launch."""
    G = TO._grid()
    units = BF16_UNITS
    k1, b1, k10, b10 = _w(12, (3, 3, 64, 64), 20.0), _bias(12), _w(13, (1, 1, 64 * T, 64), 20.0), _bias(13)
    if form == "plain":
        call = lambda x, o1, ob, n: ops.conv1_conv10_bf16(x, k1, b1, k10, b10, T, out1=o1, base=ob)  # noqa: E731
    elif form == "split":
        units, _ = _split_units(units, H0, W0)

        def call(x, o1, ob, n):
            nch = TO._chains(n, H0, W0)
            R = nch % G
            ops.conv1_conv10_bf16_ex(x, k1, b1, k10, b10, T, split=(nch - R, 3, 1) if 0 < 3 * R <= G else (0, 0, 0), out1=o1, base=ob)
    else:
        call = lambda x, o1, ob, n: ops.conv1_conv10_bf16_ex(x, k1, b1, k10, b10, T, mfma=int(form[4:]), out1=o1, base=ob)  # noqa: E731
    bf = torch.bfloat16

    def spec(I1, O1):
        return {"out1": TB.ref_conv3(I1["x"].float(), k1, b1, True), "base": TB._base_ref(O1["out1"], k10, b10, T)}

    c = Case(f"conv1_conv10_bf16[{form}]", units, {"x": (T, ROW16, bf)}, {"out1": (T, ROW16, bf), "base": (1, ROW16, bf)},
             lambda I, O, n: call(I["x"], O["out1"], O["base"], n), spec, {"out1": ("bf16", None), "base": ("bf16", None)},
             staging=lambda u: 1 << 28)
    c.spec_sees_outputs = True
    run_case(c)


def test_conv3x3_accum_bf16_past_4g():
    """convmerge1 on bf16 operands, fp32 out [clips, H, W, 64]: the input of 14 532 items crosses 2^32 bytes."""
    cout = 48
    k, b = _w(14, (3, 3, 64 * T, cout), math.sqrt(576 * T)), _bias(14, cout)

    def spec(I1):
        cat = I1["x"].float().reshape(1, T, H0, W0, 64).permute(0, 2, 3, 1, 4).reshape(1, H0, W0, T * 64)
        y = F.leaky_relu(F.conv2d(cat.permute(0, 3, 1, 2), TB.r16(torch.from_numpy(k)).permute(3, 2, 0, 1), torch.from_numpy(b), padding=1), 0.2)
        return {"out": F.pad(y.permute(0, 2, 3, 1), (0, 64 - cout))}

    run_case(Case("conv3x3_accum_bf16", BF16_UNITS, {"x": (T, ROW16, torch.bfloat16)}, {"out": (1, ROW16, torch.float32)},
                  lambda I, O, n: ops.conv3x3_accum_bf16(I["x"], k, b, act=True, frames_per_clip=T, out=O["out"]), spec,
                  {"out": ("relmax", TB.ACCUM_BF16_REL_TOL)}))


def test_conv1x1_bf16_past_4g():
    k, b = _w(15, (1, 1, 64 * T, 64), 20.0), _bias(15)

    def spec(I1):
        cat = I1["x"].float().reshape(1, T, H0, W0, 64).permute(0, 2, 3, 1, 4).reshape(1, H0, W0, T * 64)
        return {"out": F.leaky_relu(cat @ TB.r16(torch.from_numpy(k[0, 0])) + torch.from_numpy(b), 0.2)}

    run_case(Case("conv1x1_bf16", BF16_UNITS, {"x": (T, ROW16, torch.bfloat16)}, {"out": (1, ROW16, torch.bfloat16)},
                  lambda I, O, n: ops.conv1x1_bf16(I["x"], k, b, act=True, frames_per_item=T, out=O["out"]), spec, {"out": ("bf16", None)}))


# ---- tier B: head and tail ---------------------------------------------------------------------------------------------------------------------------
def _k0():
    return _w(16, (5, 5, 3, 64), math.sqrt(75.0)), _bias(16)


@pytest.mark.parametrize("f32", [False, True])
def test_conv0_past_4g(f32):
    """conv0, the f16-pipe kernel and the fp32 VALU kernel: 2351 clips of 3 frames of 34 x 70 (the hook packs the frames 2 x 2 first: even
    sizes), the 64-channel output past 2^32 bytes (the frame rides in blockIdx.z).  The parts run must give the same bits: launch_nl_pack
    is one thread per element, launch_conv0 has one kernel per choice of f32 and a grid of (tiles across, tiles down, B * T): a workgroup
    owns one tile of one frame and sums its 75 taps in a fixed order."""
    units = _units_fp32(HE, WE)
    k, b = _k0()
    spec = lambda I1: {"out": torch.from_numpy(pfnl_spec.lrelu(_conv64(_f64(I1["x"]).reshape(T, HE, WE, 3), k, b)))}  # noqa: E731
    run_case(Case(f"conv0[f32={f32}]", units, {"x": (1, (T, HE, WE, 3), torch.float32, "uniform", 1.0)}, {"out": (T, (HE, WE, 64), torch.float32)},
                  lambda I, O, n: ops.conv0(I["x"], k, b, f32=f32, out=O["out"]), spec, {"out": ("relmax", TO.CONV0_REL_TOL)},
                  staging=lambda u: u * HE * WE * 64 * 4, parts_bits=True))


def test_conv0_bf16_past_4g():
    """conv0 as precision=bf16 runs it, 4702 clips: bit-equal to the bf16 rounding of conv0 on the same clip (test_gpu_bf16_numerics.py)."""
    k, b = _k0()
    units = 2 * _units_fp32(HE, WE)
    spec = lambda I1: {"out": ops.conv0(I1["x"].cuda(), k, b).to(torch.bfloat16).cpu()}  # noqa: E731
    run_case(Case("conv0_bf16", units, {"x": (1, (T, HE, WE, 3), torch.float32, "uniform", 1.0)}, {"out": (T, (HE, WE, 64), torch.bfloat16)},
                  lambda I, O, n: ops.conv0_bf16(I["x"], k, b, out=O["out"]), spec, {"out": ("bits", None)},
                  staging=lambda u: u * HE * WE * 64 * 4))


@pytest.mark.parametrize("scale", [4, 2])
def test_tail_past_4g(scale):
    """The tail: merge [B, 33, 70, 48] past 2^32 bytes (and, at scale 4, the output as well); the clip rides in blockIdx.z.  The parts run
    must give the same bits: launch_tail's grid is (tiles across, tiles down, B), one kernel per scale, a thread owns its output pixels
    and a fixed loop over the 3 x 3 x 12 taps and the bicubic taps."""
    units = big.items_for(192, H0, W0, 1, big.TIER_B)
    co = 12 if scale == 4 else 3
    k, b = _w(17, (3, 3, 12, co), math.sqrt(108.0)), _bias(17, co)

    def spec(I1):
        o = _conv64(pfnl_spec.depth_to_space2(_f64(I1["merge"])), k, b)
        if scale == 4:
            o = pfnl_spec.depth_to_space2(o)
        return {"out": torch.from_numpy((o + pfnl_spec.resize_bicubic_tf1(_f64(I1["x"])[:, T // 2], scale))[:, None])}

    run_case(Case(f"tail[x{scale}]", units, {"merge": (1, (H0, W0, 48), torch.float32), "x": (1, (T, H0, W0, 3), torch.float32, "uniform", 1.0)},
                  {"out": (1, (1, scale * H0, scale * W0, 3), torch.float32)},
                  lambda I, O, n: ops.tail(I["merge"], I["x"], k, b, scale, out=O["out"]), spec, {"out": ("abs", TO.TAIL_ABS_TOL)},
                  parts_bits=True))


def test_bicubic_past_4g():
    """bicubic_kernel: one thread per output pixel over a size_t grid-stride loop, each with its fixed 4 x 4 taps: same bits in parts."""
    units = big.items_for(192, H0, W0, 1, big.TIER_B)
    spec = lambda I1: {"out": torch.from_numpy(pfnl_spec.resize_bicubic_tf1(_f64(I1["x"]), 4))}  # noqa: E731
    run_case(Case("bicubic", units, {"x": (1, (H0, W0, 3), torch.float32, "uniform", 1.0)}, {"out": (1, (4 * H0, 4 * W0, 3), torch.float32)},
                  lambda I, O, n: ops.bicubic(I["x"], 4, out=O["out"]), spec, {"out": ("abs", TO.RESAMPLE_ABS_TOL)}, parts_bits=True))


def test_blur_decimate_past_4g():
    """blur_decimate_kernel: one thread per output pixel over a size_t grid-stride loop, a fixed tap loop: same bits in parts."""
    Hh, Wh = 4 * H0 - 1, 4 * W0 - 3                                      # ragged against the stride
    units = big.items_for(12, Hh, Wh, 1, big.TIER_B)
    spec = lambda I1: {"out": torch.from_numpy(synth.blur_decimate(_f64(I1["hr"]), 4))}  # noqa: E731
    run_case(Case("blur_decimate", units, {"hr": (1, (Hh, Wh, 3), torch.float32, "uniform", 1.0)}, {"out": (1, (H0, W0, 3), torch.float32)},
                  lambda I, O, n: ops.blur_decimate(I["hr"], 4, out=O["out"]), spec, {"out": ("abs", TO.RESAMPLE_ABS_TOL)},
                  parts_bits=True))


# ---- the non-local block ---------------------------------------------------------------------------------------------------------------------------------
NL_H, NL_W = 8, 16                                                       # N = 32 keys, npad = 96
NL_N = (NL_H // 2) * (NL_W // 2)
NLB_H, NLB_W = 32, 36                                                    # N = 288 keys: X [B][N][64] crosses 2^32 bytes at a B a grid axis holds


def _nl_weights():
    Cc = 12 * T
    rng = np.random.default_rng(21)
    mk = lambda sc: (rng.normal(size=(1, 1, Cc, Cc)) * sc).astype(np.float32)  # noqa: E731
    mb = lambda sc=0.05: (rng.normal(size=Cc) * sc).astype(np.float32)  # noqa: E731
    return mk(0.1), mb(), mk(0.1), mb(), (mk(0.15), mb(0.3)), (mk(0.15), mb(0.3))


def _nl_spec(wg, bg, ww, bw, **kw):
    f = lambda a: a.astype(np.float64)  # noqa: E731

    def spec(I1):
        x64 = _f64(I1["x"])
        stack = np.concatenate([x64[:, t] for t in range(T)], -1)
        z = pfnl_spec.nonlocal_block(pfnl_spec.space_to_depth2(stack), f(wg), f(bg), f(ww), f(bw), **kw)
        return {"out": torch.from_numpy(stack + pfnl_spec.depth_to_space2(z))}
    return spec


def _nl_case(name, B, call, spec, tol, Hh=NL_H, Ww=NL_W, f16=True):
    """The non-local hooks take clips; unit = clip.  The tensors that cross a tier are the hook's own (X [B][N][CP], the packed operands)."""
    N = (Hh // 2) * (Ww // 2)
    return Case(name, B, {"x": (1, (T, Hh, Ww, 3), torch.float32, "uniform", 1.0)}, {"out": (1, (Hh, Ww, 3 * T), torch.float32)},
                lambda I, O, n: call(I["x"], O["out"]), spec, {"out": ("abs", tol)},
                staging=lambda u: u * (2 * N * big.nl_padded_ch(12 * T) * 4 + (2 * big.nl_f16_scratch_halfs(1, N) if f16 else 0)) + (1 << 28))


def _run_nl(c, sel, nan_is_a_result=False):
    """run_case for the non-local hooks: the tensors that cross a tier are the hook's own (X [B][N][CP], the packed binary16 operands), so the
    selected clips are given by the caller; the parts run uses three slices."""
    need = big.footprint([_nbytes(c.units, v[1], v[2]) for v in list(c.ins.values()) + list(c.outs.values())], staging=c.staging(c.units),
                         parts_bytes=2 * _nbytes(c.units, c.outs["out"][1], torch.float32))
    _reserve(c.name, need)
    g = _gen(c.seed)
    x = _draw((c.units,) + tuple(c.ins["x"][1]), torch.float32, g, "uniform")
    before = _checksum(x)
    out = _nan((c.units,) + tuple(c.outs["out"][1]))
    if nan_is_a_result:                                                  # the dot-product form divides 0 by 0 for a query without a positive
        out.fill_(float("inf"))                                          # affinity, as the reference does (utils.py:61-63): the sentinel is inf
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    c.call({"x": x}, {"out": out}, c.units)
    torch.cuda.synchronize()
    TIMES[c.name] = (time.perf_counter() - t0, need)
    assert not bool(torch.isinf(out).any()) if nan_is_a_result else not _has_nan(out), f"{c.name}: not every element of out was written"
    assert _checksum(x) == before
    kind, tol = c.tol["out"]
    for u in sorted(set(sel)):
        got, ref = out[u:u + 1].cpu(), c.spec({"x": x[u:u + 1].cpu()})["out"]
        ok = torch.isfinite(ref)
        assert torch.equal(torch.isfinite(got), ok) and (nan_is_a_result or bool(ok.all())) and float(ok.double().mean()) > 0.5, (c.name, "clip", u)
        _close_spec(kind, tol, torch.where(ok, got, 0.0), torch.where(ok, ref, 0.0), (c.name, "clip", u))
    step = -(-c.units // 3)
    for u0 in range(0, c.units, step):
        u1 = min(c.units, u0 + step)
        part = _nan((u1 - u0,) + tuple(c.outs["out"][1]))
        c.call({"x": x[u0:u1]}, {"out": part}, u1 - u0)
        whole = out[u0:u1]
        if nan_is_a_result:
            ok = torch.isfinite(part)
            assert torch.equal(torch.isfinite(whole), ok), (c.name, "clips", u0, u1)
            whole, part = torch.where(ok, whole, 0.0), torch.where(ok, part, 0.0)
        _close_parts(kind, tol, whole, part, (c.name, "clips", u0, u1))  # (a bound: the key split may depend on B)


@pytest.mark.parametrize("precision", ["split16", "f16"])
@pytest.mark.parametrize("extra", [0, 1])
def test_nonlocal_f16_at_the_chunk_limit(precision, extra):
    """nl_attn_f16_sw_kernel reaches Khi, Klo, Vthi, Vtlo through ONE resource with 32-bit offsets; launch_nl_attn_f16 chunks the batch at
    0x7fff0000 bytes.  At N = 32 keys the largest B of one launch is 29 126 clips (tests/test_big_host.py): offsets up to within one clip of
    the limit, 64 KB under the out-of-range offset (tier A, unchunked).  At B + 1 the first chunk is full and the second holds one clip."""
    B = big.nl_max_batch_one_launch(NL_N) + extra
    wg, bg, ww, bw, _, _ = _nl_weights()
    tol = TO.NONLOCAL_ABS_TOL if precision == "split16" else TO.NONLOCAL_F16_ABS_TOL
    c = _nl_case(f"nonlocal_residual[{precision},B={B}]", B, lambda x, o: ops.nonlocal_residual(x, wg, bg, ww, bw, precision=precision, out=o),
                 _nl_spec(wg, bg, ww, bw), tol)
    _run_nl(c, [0, 1, B // 2, B - extra - 1, B - 1])                     # the ends of every packed array, of the first chunk, and the last clip


@pytest.mark.parametrize("hook", ["fp32", "block_dot_pooled"])
def test_nonlocal_fp32_past_4g(hook):
    """nonlocal.hip (precision fp32) and nonlocal_block(nltype = 2, sub_sample = 2) at a B for which X [B][N][CP] crosses 2^32 bytes.  The
    clip rides in gridDim.y of these kernels: at LR 8 x 16 (8 KB of X a clip) that takes 524 290 clips, more than a grid axis holds, so
    these two cases use LR 32 x 36 (N = 288 keys, 72 KB a clip, 58 256 clips)."""
    cp = big.nl_padded_ch(12 * T)
    N = (NLB_H // 2) * (NLB_W // 2)
    B = big.items_for(4 * cp, N, 1, 1, big.TIER_B)
    assert B <= big.TIER_N
    wg, bg, ww, bw, th, ph = _nl_weights()
    f = lambda a: a.astype(np.float64)  # noqa: E731
    if hook == "fp32":
        call = lambda x, o: ops.nonlocal_residual(x, wg, bg, ww, bw, precision="fp32", out=o)  # noqa: E731
        spec = _nl_spec(wg, bg, ww, bw)
    else:
        call = lambda x, o: ops.nonlocal_block(x, wg, bg, ww, bw, theta=th, phi=ph, nltype=2, sub_sample=2, out=o)  # noqa: E731
        spec = _nl_spec(wg, bg, ww, bw, theta=(f(th[0]), f(th[1])), phi=(f(ph[0]), f(ph[1])), nltype=2, sub_sample=2)
    c = _nl_case(f"nonlocal[{hook},B={B}]", B, call, spec, TO.NONLOCAL_ABS_TOL, NLB_H, NLB_W, f16=False)
    _run_nl(c, [0, B - 1] + [i for tri in big.straddlers(4 * cp, N, 1, B).values() for i in tri], nan_is_a_result=hook != "fp32")


# ---- tier B: ensemble and tiling copies (the reference: torch on the whole tensor, bit for bit) -----------------------------------------------------------
DH_N, DH_H, DH_W = 1000, 361, 997                                        # 4.32 GB; image 994 holds byte 2^32, 995 .. 999 lie beyond it


def _torch_transform(x, k):
    if k & 1:
        x = x.flip(-2)
    if k & 2:
        x = x.flip(-3)
    if k & 4:
        x = x.transpose(-3, -2)
    return x


def _torch_inverse(y, k):
    if k & 4:
        y = y.transpose(-3, -2)
    if k & 2:
        y = y.flip(-3)
    if k & 1:
        y = y.flip(-2)
    return y


def _equal_by_image(a, b, step=100):
    """torch.equal over runs of images (b may be a lazy view: each run is materialised alone)."""
    return all(torch.equal(a[i:i + step], b[i:i + step]) for i in range(0, a.shape[0], step))


@pytest.mark.parametrize("k", range(8))
def test_dihedral_past_4g(k):
    one = DH_N * DH_H * DH_W * 12
    assert big.crosses(DH_H * DH_W * 12, 1, 1, DH_N, big.TIER_B)
    _reserve(f"dihedral[{k}]", big.footprint([one, one], parts_bytes=one // 5))
    x = _draw((DH_N, DH_H, DH_W, 3), torch.float32, _gen(30 + k))
    before = _checksum(x)
    out = _nan((DH_N, DH_W, DH_H, 3) if k & 4 else (DH_N, DH_H, DH_W, 3))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ops.dihedral(x, k, out=out)
    torch.cuda.synchronize()
    TIMES[f"dihedral[{k}]"] = (time.perf_counter() - t0, 2 * one)
    assert not _has_nan(out)
    assert _equal_by_image(out, _torch_transform(x, k))
    assert _checksum(x) == before


@pytest.mark.parametrize("k", range(8))
def test_dihedral_accum_past_4g(k):
    one = DH_N * DH_H * DH_W * 12
    _reserve(f"dihedral_accum[{k}]", big.footprint([one, one, one], parts_bytes=one // 5))
    g = _gen(40 + k)
    acc = _draw((DH_N, DH_H, DH_W, 3), torch.float32, g)
    y = _draw((DH_N, DH_W, DH_H, 3) if k & 4 else (DH_N, DH_H, DH_W, 3), torch.float32, g)
    want = torch.empty_like(acc)
    for i in range(0, DH_N, 100):
        want[i:i + 100] = (acc[i:i + 100] + _torch_inverse(y[i:i + 100], k)) * 0.5     # one rounding of the sum, an exact scale
    before = _checksum(y)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ops.dihedral_accum(acc, y, k, scale=0.5)
    torch.cuda.synchronize()
    TIMES[f"dihedral_accum[{k}]"] = (time.perf_counter() - t0, 3 * one)
    assert _equal_by_image(acc, want)
    assert _checksum(y) == before


def _tile_grid(Hh, Ww, tile):
    from pfnl_amd import tiles
    th, tw, rows, cols = tiles.grid(Hh, Ww, tiles.check(Hh, Ww, tile))
    return th, tw, rows, cols


def _gather_equal(out, x, th, tw, rows, cols):
    """tiles.split on the device: tile (clip, row, col) of the stack is the window of x at the tile's origin."""
    B, Tn = x.shape[:2]
    o6 = out.view(B, len(rows), len(cols), Tn, th, tw, 3)
    return all(torch.equal(o6[:, r, c], x[:, :, oy:oy + th, ox:ox + tw]) for r, (oy, _, _) in enumerate(rows) for c, (ox, _, _) in enumerate(cols))


def _scatter_want(y, B, Hh, Ww, th, tw, rows, cols):
    """tiles.assemble at scale 1 on the device: every tile's owned rectangle at its place."""
    want = _nan((B,) + tuple(y.shape[1:-3]) + (Hh, Ww, 3))
    y6 = y.view((B, len(rows), len(cols)) + tuple(y.shape[1:]))
    for r, (oy, ay, by) in enumerate(rows):
        for c, (ox, ax, bx) in enumerate(cols):
            want[..., ay:by, ax:bx, :] = y6[:, r, c][..., ay - oy:by - oy, ax - ox:bx - ox, :]
    return want


TILE_HW, TILE = (250, 398), (96, 128, 8)                                 # 3 x 4 overlapping tiles of 96 x 128


def test_tile_gather_past_4g():
    """tile_gather: the stack of overlapping tiles of x [812, 3, 250, 398, 3] is past 2^32 bytes, x past 2^31; against slicing on the device."""
    Hh, Ww = TILE_HW
    th, tw, rows, cols = _tile_grid(Hh, Ww, TILE)
    per = T * th * tw * 12
    B = -(-(big.TIER_B // per + 2) // (len(rows) * len(cols)))
    count = B * len(rows) * len(cols)
    xb, ob = B * T * Hh * Ww * 12, count * per
    assert big.crosses(per, 1, 1, count, big.TIER_B) and xb > big.TIER_A
    _reserve("tile_gather", big.footprint([xb, ob], parts_bytes=ob // 4))
    x = _draw((B, T, Hh, Ww, 3), torch.float32, _gen(50))
    before = _checksum(x)
    out = _nan((count, T, th, tw, 3))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ops.tile_gather(x, TILE, out=out)
    torch.cuda.synchronize()
    TIMES["tile_gather"] = (time.perf_counter() - t0, xb + ob)
    assert not _has_nan(out)
    assert _gather_equal(out, x, th, tw, rows, cols)
    assert _checksum(x) == before


def test_tile_scatter_past_4g():
    """tile_scatter at scale 1: the tile results y [count, 1, 96, 128, 3] are past 2^32 bytes; against the owned rectangles placed by slicing
    on the device.  Every element of the canvas belongs to one tile: no NaN is left."""
    Hh, Ww = TILE_HW
    th, tw, rows, cols = _tile_grid(Hh, Ww, TILE)
    per = th * tw * 12
    B = -(-(big.TIER_B // per + 2) // (len(rows) * len(cols)))
    count = B * len(rows) * len(cols)
    yb, ob = count * per, B * Hh * Ww * 12
    assert big.crosses(per, 1, 1, count, big.TIER_B) and ob > big.TIER_A
    _reserve("tile_scatter", big.footprint([yb, ob, ob], parts_bytes=ob))
    y = _draw((count, 1, th, tw, 3), torch.float32, _gen(51))
    before = _checksum(y)
    canvas = _nan((B, 1, Hh, Ww, 3))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ops.tile_scatter(y, canvas, TILE, 1)
    torch.cuda.synchronize()
    TIMES["tile_scatter"] = (time.perf_counter() - t0, yb + 2 * ob)
    assert not _has_nan(canvas)
    assert torch.equal(canvas, _scatter_want(y, B, Hh, Ww, th, tw, rows, cols))
    assert _checksum(y) == before


# ---- tier C: the flat kernels (2^31 + 4096 elements; the torch expression of the documented rule, bit for bit) ----------------------------------------------
FLAT_N = big.TIER_C + 4096


def _quant_ref(x, top):
    return torch.round(torch.clamp(x * top, 0.0, top))                   # float32 product, round half to even


@pytest.mark.parametrize("bits", [8, 10])
def test_quantise_past_2g_elements(bits):
    top, dt, fn = (255.0, torch.uint8, ops.quantise_u8) if bits == 8 else (1023.0, torch.uint16, ops.quantise_u10)
    osz = 1 if bits == 8 else 2
    _reserve(f"quantise_u{bits}", big.footprint([4 * FLAT_N, osz * FLAT_N], parts_bytes=10 * CHUNK))
    x = _draw((FLAT_N,), torch.float32, _gen(60 + bits), "uniform", 1.4)
    x -= 0.2
    x[-8:] = torch.tensor([0.5 / top, 1.5 / top, 2.5 / top, (top - 0.5) / top, 1.0, 0.0, -1.0, 2.0], device="cuda")   # ties, ends, out of range
    x[big.TIER_C - 2:big.TIER_C + 2] = torch.tensor([0.5 / top, 1.5 / top, 2.5 / top, 1.0], device="cuda")
    before = _checksum(x)
    out = torch.full((FLAT_N,), 7, dtype=dt, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(x, out=out)
    torch.cuda.synchronize()
    TIMES[f"quantise_u{bits}"] = (time.perf_counter() - t0, (4 + osz) * FLAT_N)
    for i in range(0, FLAT_N, CHUNK):
        want = _quant_ref(x[i:i + CHUNK], top)
        assert torch.equal(out[i:i + CHUNK].to(torch.float32), want), i
    assert _checksum(x) == before


@pytest.mark.parametrize("src", ["float", "u8", "u10"])
def test_gather_windows_past_2g_elements(src):
    """The clamped sliding windows with an output past 2^31 elements: 1037 frames of 332 x 696 x 3, T = 3."""
    Hh, Ww, Fr = 332, 696, 1037
    per = Hh * Ww * 3
    assert Fr * T * per >= big.TIER_C + T * per
    isz = {"float": 4, "u8": 1, "u10": 2}[src]
    _reserve(f"gather_windows[{src}]", big.footprint([isz * Fr * per, 4 * Fr * T * per], parts_bytes=8 * T * per * 16))
    g = _gen(70)
    if src == "float":
        fr = _draw((Fr, Hh, Ww, 3), torch.float32, g, "uniform")
        deq = lambda t: t  # noqa: E731
    elif src == "u8":
        fr = torch.randint(0, 256, (Fr, Hh, Ww, 3), generator=g, device="cuda", dtype=torch.uint8)
        deq = lambda t: (t.to(torch.float64) / 255.0).to(torch.float32)  # noqa: E731
    else:
        fr = torch.randint(0, 1100, (Fr, Hh, Ww, 3), generator=g, device="cuda", dtype=torch.int16).view(torch.uint16)
        deq = lambda t: (t.to(torch.int32).clamp(max=1023).to(torch.float64) / 1023.0).to(torch.float32)  # noqa: E731
    before = _checksum(fr)
    out = _nan((Fr, T, Hh, Ww, 3))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if src == "float":
        ops.gather_windows(fr, 0, Fr, T, out=out)
    elif src == "u8":
        ops.gather_windows_u8(fr, Fr - 1, 0, Fr, T, out=out)             # a ring of Fr slots, frame f in slot f
    else:
        ops.gather_windows_u10(fr, Fr - 1, 0, Fr, T, out=out)
    torch.cuda.synchronize()
    TIMES[f"gather_windows[{src}]"] = (time.perf_counter() - t0, (isz + 4 * T) * Fr * per)
    assert not _has_nan(out)
    idx = (torch.arange(Fr, device="cuda")[:, None] + torch.arange(T, device="cuda")[None, :] - T // 2).clamp(0, Fr - 1)
    for i in range(0, Fr, 16):
        rows = (fr.view(torch.int16) if src == "u10" else fr)[idx[i:i + 16].reshape(-1)]      # (torch indexes no uint16: the same bits, below 2^15)
        assert torch.equal(out[i:i + 16], deq(rows).view(-1, T, Hh, Ww, 3)), i
    assert _checksum(fr) == before


# ---- tier N: more items than a grid axis holds ------------------------------------------------------------------------------------------------------------------
def _served_or_refused(name, call, out, check):
    """The hook serves every item, or returns an error from the C-ABI with the output untouched; a partial result is a bug."""
    try:
        call()
    except _capi.PFNLHipError:
        torch.cuda.synchronize()
        if out.is_floating_point():
            assert _all_nan(out), f"{name}: refused, but part of the output was written"
        else:
            assert bool((out == 7).all()), f"{name}: refused, but part of the output was written"
        return
    torch.cuda.synchronize()
    check()


def test_conv0_more_frames_than_a_grid_axis():
    B = big.N_ITEMS // T                                                 # 21 846 clips: 65 538 frames in grid z
    k, b = _k0()
    _reserve("conv0[N]", big.footprint([B * T * 2 * 2 * 12, 3 * B * T * 2 * 2 * 256], staging=B * 64 * 4 + B * T * 2 * 2 * 256))
    x = _draw((B, T, 2, 2, 3), torch.float32, _gen(80), "uniform")
    out = _nan((B * T, 2, 2, 64))

    def check():
        assert not _has_nan(out)
        for u in (0, 1, (big.TIER_N // T) - 1, big.TIER_N // T, B - 2, B - 1):
            ref = pfnl_spec.lrelu(_conv64(_f64(x[u].cpu()), k, b))
            _close_spec("relmax", TO.CONV0_REL_TOL, out[u * T:(u + 1) * T].cpu(), torch.from_numpy(ref), ("conv0", u))
        h = B // 2
        parts = torch.cat([ops.conv0(x[:h], k, b), ops.conv0(x[h:], k, b)])
        assert torch.equal(out, parts), "conv0 in halves"                # (one workgroup per tile of one frame: test_conv0_past_4g)
    _served_or_refused("conv0", lambda: ops.conv0(x, k, b, out=out), out, check)


def test_tail_more_clips_than_a_grid_axis():
    B = big.N_ITEMS
    k, b = _w(17, (3, 3, 12, 12), math.sqrt(108.0)), _bias(17, 12)
    _reserve("tail[N]", big.footprint([B * 4 * 192, B * T * 4 * 12, 3 * B * 64 * 12]))
    g = _gen(81)
    merge, x = _draw((B, 2, 2, 48), torch.float32, g), _draw((B, T, 2, 2, 3), torch.float32, g, "uniform")
    out = _nan((B, 1, 8, 8, 3))

    def check():
        assert not _has_nan(out)
        for u in (0, big.TIER_N - 1, big.TIER_N, big.TIER_N + 1, B - 1):
            o = pfnl_spec.depth_to_space2(_conv64(pfnl_spec.depth_to_space2(_f64(merge[u:u + 1].cpu())), k, b))
            ref = (o + pfnl_spec.resize_bicubic_tf1(_f64(x[u:u + 1, T // 2].cpu()), 4))[:, None]
            _close_spec("abs", TO.TAIL_ABS_TOL, out[u:u + 1].cpu(), torch.from_numpy(ref), ("tail", u))
        h = B // 2
        parts = torch.cat([ops.tail(merge[:h], x[:h], k, b, 4), ops.tail(merge[h:], x[h:], k, b, 4)])
        assert torch.equal(out, parts), "tail in halves"
    _served_or_refused("tail", lambda: ops.tail(merge, x, k, b, 4, out=out), out, check)


def test_resize_more_frames_than_a_grid_axis():
    """resize_u8 / resize_place_u8 (frame in grid z, launched in runs of 65535): the frames around index 65535, the first and the last byte
    for byte the host rule (pfnl_amd/resize.py resize, pfnl_amd/fit.py place), and the whole output the same frames resized in two halves."""
    from pfnl_amd import fit, resize
    n = big.N_ITEMS
    _reserve("resize[N]", big.footprint([n * 4 * 6 * 3, 3 * n * 6 * 5 * 3]))
    fr = torch.randint(0, 256, (n, 4, 6, 3), generator=_gen(82), device="cuda", dtype=torch.uint8)
    h = n // 2
    dst = (1, 1, 4, 3)                                                   # the frame at 4 x 3 inside the 6 x 5 canvas, fill around it
    rules = {"resize_u8": lambda f: resize.resize(f, 6, 5), "resize_place_u8": lambda f: fit.place(f, 6, 5, None, dst, (1, 2, 3))}
    for name, fn in (("resize_u8", lambda f, o: ops.resize_u8(f, (6, 5), out=o)),
                     ("resize_place_u8", lambda f, o: ops.resize_place_u8(f, (6, 5), dst=dst, fill=(1, 2, 3), out=o))):
        out = torch.full((n, 6, 5, 3), 7, dtype=torch.uint8, device="cuda")

        def check():
            for i in (0, 1, big.TIER_N - 2, big.TIER_N - 1, big.TIER_N, big.TIER_N + 1, n - 1):
                assert np.array_equal(out[i].cpu().numpy(), rules[name](fr[i].cpu().numpy())), (name, i)
            parts = torch.cat([fn(fr[:h], None), fn(fr[h:], None)])
            assert torch.equal(out, parts), name
        _served_or_refused(name, lambda: fn(fr, out), out, check)


def test_score_y_more_frames_than_a_grid_axis():
    """score_y carries the frame in grid y and says so: F > 65535 is refused on the host (pfnl_op_score_y checks F before any launch)."""
    n = big.N_ITEMS
    _reserve("score_y[N]", big.footprint([n * 16 * 16 * 3, n * 32]))
    g = _gen(83)
    a = torch.randint(0, 256, (n, 16, 16, 3), generator=g, device="cuda", dtype=torch.uint8)
    out = _nan((n, 4), torch.float64)
    with pytest.raises(_capi.PFNLHipError, match="65535"):
        ops.score_y(a, a, out=out)
    torch.cuda.synchronize()
    assert _all_nan(out)


def test_tile_gather_scatter_more_images_than_a_grid_axis():
    """tile_gather (image = clip x frame in grid y) and tile_scatter (tile in grid y), launched in runs of 65535."""
    B, Hh, Ww, tile = big.N_ITEMS // T, 16, 24, (16, 16, 4)
    th, tw, rows, cols = _tile_grid(Hh, Ww, tile)
    nt = len(rows) * len(cols)
    _reserve("tiles[N]", big.footprint([B * T * Hh * Ww * 12, B * nt * T * th * tw * 12, big.N_ITEMS * nt * th * tw * 12, 3 * big.N_ITEMS * Hh * Ww * 12]))
    x = _draw((B, T, Hh, Ww, 3), torch.float32, _gen(84))
    out = _nan((B * len(rows) * len(cols), T, th, tw, 3))

    def check():
        assert not _has_nan(out)
        assert _gather_equal(out, x, th, tw, rows, cols)
    _served_or_refused("tile_gather", lambda: ops.tile_gather(x, tile, out=out), out, check)
    Bs = big.N_ITEMS                                                     # scatter: 65 538 frames, more tiles still
    y = _draw((Bs * len(rows) * len(cols), 1, th, tw, 3), torch.float32, _gen(85))
    canvas = _nan((Bs, 1, Hh, Ww, 3))

    def check_scatter():
        assert not _has_nan(canvas)
        assert torch.equal(canvas, _scatter_want(y, Bs, Hh, Ww, th, tw, rows, cols))
    _served_or_refused("tile_scatter", lambda: ops.tile_scatter(y, canvas, tile, 1), canvas, check_scatter)


# ---- the forward --------------------------------------------------------------------------------------------------------------------------------------------------
import test_gpu_forward as TF  # noqa: E402   (ABS_TOL)
from oracle import pfnl_fast  # noqa: E402
from pfnl_amd.engine import PFNLEngine  # noqa: E402
from pfnl_amd.spec import PFNLGeometry  # noqa: E402

FWD_H = FWD_W = 32
# test_gpu_bf16.py holds a bf16 forward to FORWARD_PSNR_DB against the equally rounded oracle at B = 1 as well as on batches, so the bound
# holds for one clip.  Two forwards of a clip within it of one oracle: rmse(a, b) <= rmse(a, o) + rmse(b, o), twice the rmse, 20 log10(2) dB
# less - per clip, and asserted on the worst clip, so that one clip from another clip's place cannot hide in an average over thousands
FORWARD_BF16_PARTS_PSNR_DB = TB.FORWARD_PSNR_DB - 20.0 * math.log10(2.0)


def _min_clip_psnr(a, b):
    """The lowest PSNR of any one clip of a against the same clip of b ([n, ...] each, values on the [0, 1] scale)."""
    mse = float(((a.double() - b.double()) ** 2).flatten(1).mean(1).max())
    return float("inf") if mse == 0.0 else -10.0 * math.log10(mse)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_forward_past_4g(precision):
    """PFNLEngine.forward on device pointers, num_block = 2, T = 3, LR 32 x 32, at the clip count that carries the 64-channel activations
    [B * 3, 32, 32, 64] past 2^32 bytes: 5465 clips at fp32 (256 bytes a pixel), 10 926 at precision = bf16 (128).  The plan is the chained
    structure; the workspace is finite and holds at least two such activations; the clips at the activation's thresholds, the first and
    the last against the FastOracle; the whole output against the same engine over three sub-batches (bf16: clip by clip, the worst clip).  At bf16 the output itself passes
    2^31 bytes: one host-pointer call (numpy in, numpy out, through the pinned strips) must give the device call's bytes."""
    bf = precision == "bf16"
    bpp = 128 if bf else 256
    B = -(-big.TIER_B // (T * FWD_H * FWD_W * bpp)) + 3
    assert B == (10926 if bf else 5465)
    geom = PFNLGeometry(num_frames=T, scale=4, num_block=2)
    w = synth.synthetic_weights(geom, seed=T)
    eng = PFNLEngine(geom, device=0)
    try:
        eng.load_weights(w)
        if bf:
            eng.set_option("precision", "bf16")
        pl = eng.plan(B, FWD_H, FWD_W)
        print(f"forward[{precision}] B={B}: {eng.plan_text(B, FWD_H, FWD_W)}")
        assert pl["structure"] in (("bf16_3", "bf16_3_split") if bf else ("chain2", "chain2_split", "chain2_sf0")), pl
        # the chained structure: conv1_i + conv10_i in one launch, the whole of conv2_i in the other (bf16_3: the per-frame half of conv2_i is
        # a third), and c10_finalize_kernel (c1x1 = 1) exactly where the last round of chains is cut
        cut = pl["structure"].endswith("_split")
        assert pl["launches_per_block"] == (3 if bf else 2) + pl["c1x1"] and pl["c1x1"] == (1 if cut else 0), pl
        assert pl["chains"] == B * TO._chains(1, FWD_H, FWD_W)
        if cut:
            assert pl["split_parts"] >= 2 and pl["split_parts"] * pl["part_frames"] >= T and 0 < pl["whole_chains"] < pl["chains"], pl
            assert (pl["chains"] - pl["whole_chains"]) * pl["split_parts"] <= TO._grid() and pl["whole_chains"] % TO._grid() == 0, pl
        else:
            assert pl["whole_chains"] == pl["chains"] and pl["split_parts"] == 0, pl
        act = B * T * FWD_H * FWD_W * bpp
        ws = eng.workspace_bytes(B, FWD_H, FWD_W)
        # what a forward of this shape holds under any plan (pfnl_workspace_bytes, capi.hip): X and Xo [B][N][CP] fp32 of the non-local block,
        # the two trunk activations inp0 and inp1 at the precision's bytes per pixel, base and merge1 [B, H, W, 64] (merge1 fp32), the two
        # staging tensors; and, where the plan cuts chains, one [8][32][64] fp32 tile of raw sums per part of every cut chain
        npix = B * FWD_H * FWD_W
        named = (2 * (npix // 4) * big.nl_padded_ch(12 * T) * 4 + 2 * act + npix * (bpp + 256) + npix * T * 12 + npix * 16 * 12
                 + ((pl["chains"] - pl["whole_chains"]) * pl["split_parts"] * 8 * 32 * 64 * 4 if cut else 0))
        assert named <= ws < big.MAX_CASE_BYTES, (ws, named)
        xb, ob = B * T * FWD_H * FWD_W * 12, B * 16 * FWD_H * FWD_W * 12
        _reserve(f"forward[{precision}]", big.footprint([xb, ob], staging=ws, parts_bytes=3 * ob))
        x = _draw((B, T, FWD_H, FWD_W, 3), torch.float32, _gen(90), "uniform")
        before = _checksum(x)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        y = eng.forward(x)
        eng.sync()
        torch.cuda.synchronize()
        TIMES[f"forward[{precision}]"] = (time.perf_counter() - t0, xb + ob + ws)
        assert not _has_nan(y) and _checksum(x) == before
        fo = pfnl_fast.FastOracle(w, T, 4, 2, trunk_dtype="bf16") if bf else pfnl_fast.FastOracle(w, T, 4, 2)
        sel = sorted({i // T for i in big.selected_items(bpp, FWD_H, FWD_W, B * T)})
        ref = torch.from_numpy(np.asarray(fo.forward(x[sel].cpu().numpy()), dtype=np.float32))
        got = y[sel].cpu()
        if bf:                                                           # clip by clip: a clip from another clip's place is below 20 dB
            worst = _min_clip_psnr(got, ref)
            print(f"forward[bf16]: worst selected clip against the oracle {worst:.2f} dB")
            assert worst > TB.FORWARD_PSNR_DB, (sel, worst)
        else:
            e = float((got - ref).abs().max())
            assert e < TF.ABS_TOL, (sel, e)
        step = -(-B // 3)
        for b0 in range(0, B, step):
            part = eng.forward(x[b0:b0 + step])
            eng.sync()
            if bf:
                p = _min_clip_psnr(y[b0:b0 + step], part)
                print(f"forward[bf16]: clips {b0} ..: worst clip against the run in parts {p:.2f} dB")
                assert p > FORWARD_BF16_PARTS_PSNR_DB, (b0, p)
            else:
                _close_parts("abs", TF.ABS_TOL, y[b0:b0 + step], part, ("forward", b0))
            del part
        if bf:
            assert ob > big.TIER_A
            yh = eng.forward(x.cpu().numpy())
            assert isinstance(yh, np.ndarray) and yh.nbytes == ob
            yd = y.cpu().numpy()
            assert np.array_equal(yh.view(np.uint32), yd.view(np.uint32))
    finally:
        eng.close()


# ---- the last test: on a device this large nothing may have skipped ---------------------------------------------------------------------------------------------------
def test_zz_nothing_skipped_on_a_large_device():
    _, total = torch.cuda.mem_get_info()
    for name, (sec, need) in sorted(TIMES.items()):
        print(f"{name}: {sec:.3f} s, {need / 2 ** 30:.2f} GiB")
    if total >= 128 << 30:
        assert not _SKIPPED, f"skipped for want of memory on a device of {total} bytes: {_SKIPPED}"
