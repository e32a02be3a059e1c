"""A forward does not depend on what its handle ran before, and a kernel reads nothing outside its operands (DESIGN.md "What a forward
may depend on"; helpers and their host tests: tests/history.py, tests/test_history_host.py).

A. PFNLEngine.forward, one target per trunk structure trunk_plan can name (shapes found by asking pfnl_plan on this device): the target
   on a new engine (y0: finite, and inside the existing forward tests' bound against the oracle - so that "both runs equally wrong"
   cannot pass), a HISTORY on the same engine, the target again: bit-identical to y0.
B. The chained kernels' op hooks and forward_device with their operands inside one NaN-flooded allocation: same bits as on ordinary
   operands, the existing op tests' bound against the spec, every gap intact, every output element written.

Every case prints one line (pytest -s): structure, history, verdict."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import history as Hy  # noqa: E402
import test_gpu_bf16 as TB  # noqa: E402   (FORWARD_PSNR_DB, close_bf16 and the torch references of the bf16 op tests)
import test_gpu_forward as TF  # noqa: E402   (ABS_TOL)
import test_gpu_ops as TO  # noqa: E402   (SPLIT16_OP_REL_TOL, the fp64 reference of the chain launch, the split geometries)
from oracle import pfnl_fast, pfnl_spec  # noqa: E402
from pfnl_amd import ops, synth  # noqa: E402
from pfnl_amd.engine import PFNLEngine  # noqa: E402
from pfnl_amd.spec import PFNLGeometry  # noqa: E402

NB = 2                                            # PF blocks: block 1 reads what block 0 wrote (the split-format copy of split16_sf0 needs two)
_cache = {}


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _geom(t):
    return PFNLGeometry(num_frames=t.T, num_block=NB)


def _weights(t):
    key = ("w", t.T, t.theta)
    if key not in _cache:
        w = synth.synthetic_weights(_geom(t), seed=0)
        _cache[key] = Hy.theta_phi(_geom(t), w) if t.theta else w
    return _cache[key]


def _defaults():
    if "defaults" not in _cache:
        e = PFNLEngine(PFNLGeometry(num_block=NB), device=0)
        _cache["defaults"] = Hy.read_defaults(e)
        e.close()
    return _cache["defaults"]


def _shape(t):
    """The target's shape on this device, from pfnl_plan (a handle without weights plans as one with them)."""
    key = ("shape", t.name)
    if key not in _cache:
        e = PFNLEngine(_geom(t), device=0)
        Hy.apply_options(e, _defaults(), t.options)
        _cache[key] = Hy.find_shape(t, lambda shapes: [e.plan(*s) for s in shapes], _ncu())
        e.close()
    s = _cache[key]
    if s is None:
        # the cap (history.shape_cap: 2.5 rounds of chains on the persistent grid, derived from trunk_plan's thresholds) holds every structure
        # on the 256-CU device - a condition; elsewhere only the two chain2 targets whose rule reads chains >= grid may be out of reach
        assert _ncu() != 256 and t.name in Hy.MAY_BE_OUT_OF_REACH, f"{t.name}: no shape under {Hy.shape_cap(_ncu())} chains reaches {t.structure}"
        pytest.skip(f"{t.name}: no shape under {Hy.shape_cap(_ncu())} chains reaches {t.structure} on {_ncu()} CUs")
    return s


def _engine(t):
    e = PFNLEngine(_geom(t), device=0)
    e.load_weights(_weights(t))
    Hy.apply_options(e, _defaults(), t.options)
    B, H, W = _shape(t)
    pl = e.plan(B, H, W)
    assert Hy.matches(t, pl, _ncu()), (t.name, e.plan_text(B, H, W))      # the structure found is the one wanted
    return e


def _case(t):
    """The target's clip (host and device) and its oracle result, computed once."""
    key = ("case", t.name)
    if key not in _cache:
        B, H, W = _shape(t)
        x = synth.uniform_clips(B, t.T, H, W, seed=11 + B)
        w = _weights(t)
        opts = dict(t.options)
        if t.theta or "nl_sub_sample" in opts:                             # the general non-local family: the fp64 spec takes the arguments
            ref = pfnl_spec.forward(x, w, num_block=NB, nltype=int(opts.get("nl_type", 1)), sub_sample=int(opts.get("nl_sub_sample", 1)))
        else:
            ref = pfnl_fast.FastOracle(w, t.T, 4, NB, trunk_dtype="bf16" if t.bf16 else "fp32").forward(x)
        _cache[key] = (x, torch.from_numpy(x).cuda(), ref)
    return _cache[key]


def _judge(t, y0):
    """y0 finite and inside the bound of the existing forward test of its precision."""
    _, _, ref = _case(t)
    assert y0.shape == ref.shape and np.isfinite(y0).all(), t.name
    if t.bf16:
        p = synth.psnr(y0, ref)
        assert p > TB.FORWARD_PSNR_DB, (t.name, p)
        return "PSNR %.1f dB" % p
    err = float(np.abs(y0 - ref).max())
    assert err < TF.ABS_TOL, (t.name, err)
    return "max err %.2g" % err


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _ctx(t, others=False):
    ctx = Hy.Ctx(t, _shape(t), _defaults(), _weights(t))
    if others:
        for o in Hy.TARGETS:
            if o.name != t.name and o.T == t.T and o.theta == t.theta:        # (what this engine's geometry and weights can run)
                key = ("shape", o.name)
                if key not in _cache:
                    try:
                        _shape(o)
                    except pytest.skip.Exception:
                        pass
                if _cache.get(key):
                    ctx.others.append((o, _cache[key]))
    return ctx


def _report(t, history, verdict, extra=""):
    B, H, W = _shape(t)
    print(f"\n[history] {t.name:16s} {t.structure:13s} {B}x{t.T}x{H}x{W}  {history:22s} {verdict}  {extra}", end="")


# ---- A. histories 1 and 2: every target ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["same", "other"])
@pytest.mark.parametrize("kind", Hy.FLOODS)
@pytest.mark.parametrize("name", [t.name for t in Hy.TARGETS])
def test_forward_after_a_flood(name, kind, precision):
    """Histories 1 and 2: a device-pointer forward of an all-NaN / all-Inf / 1e4-noise clip at B + 1 clips of (H + 10) x (W + 22), in the
    target's precision and in the other one, leaves every workspace buffer's head AND tail flooded (the taps of the trunk and of
    convmerge1 show it); the target's bits do not change."""
    t = Hy.target(name)
    _, xd, _ = _case(t)
    eng = _engine(t)
    y0 = Hy.run_device(eng, xd)
    verdict = _judge(t, y0)
    ctx = _ctx(t)
    (Hy.flood if precision == "same" else Hy.flood_other_precision)(eng, ctx, kind)
    y1 = Hy.run_device(eng, xd)
    same = _same_bits(y0, y1)
    _report(t, f"flood-{kind}-{precision}", "identical" if same else "DIFFERENT", verdict)
    assert same, (name, kind, precision, int((y0 != y1).sum()), float(np.nanmax(np.abs(y0 - y1))), int((~np.isfinite(y1)).sum()))
    assert eng.range_flagged() is False                                    # the target raised no flag of its own
    eng.close()


# ---- A. histories 3 - 7: one target per trunk family ---------------------------------------------------------------------------------

def _history_plans_up(eng, ctx):
    Hy.other_plans(eng, ctx, descending=False)


def _history_plans_down(eng, ctx):
    Hy.other_plans(eng, ctx, descending=True)


HISTORIES = {"plans-ascending": _history_plans_up, "plans-descending": _history_plans_down, "range-rerun": Hy.range_rerun, "strip": Hy.strip,
             "session": Hy.session}


@pytest.mark.parametrize("history", list(HISTORIES))
@pytest.mark.parametrize("name", [t.name for t in Hy.family_targets()])
def test_forward_after_other_work(name, history):
    """Histories 3, 4, 5 and 7 on one target of each family: every other target's plan on finite clips (smaller to larger and back: the
    c10part slot count, the merge stride, the key split and the nl16 layout all change under the target); a range rerun on the f32-MFMA
    kernels (exactly one, and none for the target); a flooded strip (Xo written for the strip's queries only); a streaming session."""
    t = Hy.target(name)
    _, xd, _ = _case(t)
    eng = _engine(t)
    y0 = Hy.run_device(eng, xd)
    verdict = _judge(t, y0)
    ctx = _ctx(t, others=history.startswith("plans"))
    HISTORIES[history](eng, ctx)
    reruns = eng.range_reruns()
    y1 = Hy.run_device(eng, xd)
    same = _same_bits(y0, y1)
    _report(t, history, "identical" if same else "DIFFERENT", verdict + (f", {len(ctx.others)} plans" if ctx.others else ""))
    assert same, (name, history, int((y0 != y1).sum()), float(np.nanmax(np.abs(y0 - y1))))
    assert eng.range_reruns() == reruns and eng.range_flagged() is False
    if history.startswith("plans"):
        assert len(ctx.others) >= 14
    eng.close()


@pytest.mark.parametrize("name", [t.name for t in Hy.family_targets()])
def test_forward_graph_cache_after_a_flood(name):
    """History 6: graph=on - the target eager, captured, replayed; a flood at a shape that makes the buffers move (the captured graph
    holds raw pointers: it must be dropped); the target twice more.  All five equal the eager result of graph=off."""
    t = Hy.target(name)
    _, xd, _ = _case(t)
    eng = _engine(t)
    y0 = Hy.run_device(eng, xd)
    verdict = _judge(t, y0)
    eng.set_option("graph", "on")
    ys = [Hy.run_device(eng, xd) for _ in range(3)]
    Hy.flood(eng, _ctx(t), "nan")
    ys += [Hy.run_device(eng, xd) for _ in range(2)]
    same = [_same_bits(y0, y) for y in ys]
    _report(t, "graph-cache", "identical" if all(same) else "DIFFERENT", verdict)
    assert all(same), (name, same)
    eng.close()


# ---- B. operands inside a flooded arena ------------------------------------------------------------------------------------------------

def _grid():
    return Hy.persistent_grid(_ncu())


# 1 x 1; one ragged tile; an exact multiple of the tile; two clips whose chains end in a partial round of the grid (12 chains); T, clips, H, W
GEOMS = [(7, 1, 1, 1), (7, 1, 9, 33), (7, 1, 16, 64), (5, 2, 10, 38)]
SPLITS = ["T7-s2-uneven", "nfull0-ragged", "T3-q1"]                       # of test_conv2_chain_split_chains_op / test_bf16_v3_split_chains_op


def _geometry(g):
    """(T, clips, H, W, split) of a GEOMS entry or a named split geometry (test_gpu_ops._split_case on this device's grid)."""
    if isinstance(g, str):
        return TO._split_case(g, _grid())
    return g + ((0, 0, 0),)


def _sel(T, clips, H, W, split):
    """The clips the spec runs on (test_gpu_ops._split_subset's rule)."""
    return list(range(clips)) if clips * T * H * W <= 120000 else sorted({clips - 1, split[0] // TO._chains(1, H, W)})


def _gid(g):
    return g if isinstance(g, str) else "x".join(map(str, g))


def _arena_of(inputs, outputs, dtype, frame_elems):
    ops_ = {k: (tuple(v.shape), dtype, v) for k, v in inputs.items()}
    ops_.update({k: (tuple(s), dtype, None) for k, s in outputs.items()})
    return Hy.Arena(ops_, frame_elems * Hy.ITEMSIZE[dtype])


def _arena_verdict(label, a, plain, arena_out):
    torch.cuda.synchronize()
    r = a.check()
    same = all(torch.equal(p.view(torch.int16), q.view(torch.int16)) for p, q in zip(plain, arena_out))
    print(f"\n[arena] {label:60s} {'identical' if same else 'DIFFERENT'}; {r}", end="")
    assert r.ok, f"{label}: {r}"
    assert same, label


def _rel(got, ref):
    return float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max()))


@pytest.mark.parametrize("g,mfma", [(g, m) for m in (32, 16) for g in GEOMS + (SPLITS if m == 32 else [])], ids=lambda v: _gid(v) if not isinstance(v, int) else f"mfma{v}")
def test_conv2_chain_in_arena(g, mfma):
    """pfnl_op_conv2_chain_ex (conv3x3_sf_chain_kernel / conv3x3_sf_chain16_kernel; the cut launch on 32x32x16 only: the 16x16x32 kernel has
    no split form, test_split_chain_hooks_refuse_bad_geometries)."""
    T, clips, H, W, split = _geometry(g)
    rng = np.random.default_rng(T * 100 + H + W)
    F = clips * T
    x, res = (rng.normal(size=(F, H, W, 64)).astype(np.float32) for _ in range(2))
    base = rng.normal(size=(clips, H, W, 64)).astype(np.float32)
    k2 = (rng.normal(size=(3, 3, 128, 64)) / 34.0).astype(np.float32)
    b = (rng.normal(size=64) * 0.1).astype(np.float32)
    plain = ops.conv2_chain_ex(TO.dev(x), k2, b, TO.dev(base), TO.dev(res), T, mfma=mfma, split=split)
    a = _arena_of({"x": torch.from_numpy(x), "base": torch.from_numpy(base), "resid": torch.from_numpy(res)}, {"out": x.shape}, "float32", H * W * 64)
    got = ops.conv2_chain_ex(a["x"], k2, b, a["base"], a["resid"], T, mfma=mfma, split=split, out=a["out"])
    _arena_verdict(f"conv2_chain_ex mfma={mfma} {_gid(g)}", a, [plain], [got])
    sel = _sel(T, clips, H, W, split)
    e = _rel(TO._frames_of(got.cpu().numpy(), T, sel), TO._chain_ref(x, base, res, k2, b, T, sel))
    assert e < TO.SPLIT16_OP_REL_TOL, e


def _c1c10_data(T, clips, H, W):
    rng = np.random.default_rng(T * 10 + H * 3 + W)
    x = rng.normal(size=(clips * T, H, W, 64)).astype(np.float32)
    k1 = (rng.normal(size=(3, 3, 64, 64)) / 24.0).astype(np.float32)
    b1 = (rng.normal(size=64) * 0.1).astype(np.float32)
    k10 = (rng.normal(size=(1, 1, 64 * T, 64)) / np.sqrt(64 * T)).astype(np.float32)
    b10 = (rng.normal(size=64) * 0.1).astype(np.float32)
    return x, k1, b1, k10, b10


def _c1c10_check(x, k1, b1, k10, b10, T, sel, out1, base):
    """test_conv1_conv10_split_chains_op's fp64 spec and bound"""
    H, W = x.shape[1:3]
    ref1 = pfnl_spec.lrelu(pfnl_spec.conv2d_same(TO._frames_of(x, T, sel).astype(np.float64), k1.astype(np.float64), b1.astype(np.float64)))
    cat = ref1.reshape(len(sel), T, H, W, 64).transpose(0, 2, 3, 1, 4).reshape(len(sel), H, W, T * 64)
    refb = pfnl_spec.lrelu(pfnl_spec.conv2d_same(cat, k10.astype(np.float64), b10.astype(np.float64)))
    e1, eb = _rel(TO._frames_of(out1.cpu().numpy(), T, sel), ref1), _rel(base.cpu().numpy()[sel], refb)
    assert e1 < TO.SPLIT16_OP_REL_TOL and eb < TO.SPLIT16_OP_REL_TOL, (e1, eb)


@pytest.mark.parametrize("g,hook", [(g, h) for h in ("ex", "mfma16") for g in GEOMS + (SPLITS if h == "ex" else [])], ids=_gid)
def test_conv1_conv10_split16_in_arena(g, hook):
    """pfnl_op_conv1_conv10_split16_ex (32x32x16, whole and cut chains) and pfnl_op_conv1_conv10_split16_mfma at 16x16x32 (uncut launches
    only: ops.conv1_conv10_split16_mfma)."""
    T, clips, H, W, split = _geometry(g)
    x, k1, b1, k10, b10 = _c1c10_data(T, clips, H, W)
    call = (lambda xx, **kw: ops.conv1_conv10_split16_ex(xx, k1, b1, k10, b10, T, split=split, **kw)) if hook == "ex" else \
        (lambda xx, **kw: ops.conv1_conv10_split16_mfma(xx, k1, b1, k10, b10, T, mfma=16, **kw))
    plain = call(TO.dev(x))
    a = _arena_of({"x": torch.from_numpy(x)}, {"out1": x.shape, "base": (clips, H, W, 64)}, "float32", H * W * 64)
    got = call(a["x"], out1=a["out1"], base=a["base"])
    _arena_verdict(f"conv1_conv10_split16_{hook} {_gid(g)}", a, plain, got)
    _c1c10_check(x, k1, b1, k10, b10, T, _sel(T, clips, H, W, split), *got)


@pytest.mark.parametrize("g", GEOMS + SPLITS, ids=_gid)
def test_conv3x3_accum_split16_in_arena(g):
    """pfnl_op_conv3x3_accum_split16_ex (convmerge1 on the split-f16 kernel, cout 48; the cut launch + c10_finalize_kernel)."""
    T, clips, H, W, split = _geometry(g)
    rng = np.random.default_rng(T * 7 + H + W)
    cout = 48
    x = rng.normal(size=(clips * T, H, W, 64)).astype(np.float32)
    k = (rng.normal(size=(3, 3, 64 * T, cout)) / np.sqrt(576 * T)).astype(np.float32)
    b = (rng.normal(size=cout) * 0.1).astype(np.float32)
    plain = ops.conv3x3_accum_split16_ex(TO.dev(x), k, b, act=True, frames_per_clip=T, split=split)
    a = _arena_of({"x": torch.from_numpy(x)}, {"out": (clips, H, W, 64)}, "float32", H * W * 64)
    got = ops.conv3x3_accum_split16_ex(a["x"], k, b, act=True, frames_per_clip=T, split=split, out=a["out"])
    _arena_verdict(f"conv3x3_accum_split16_ex {_gid(g)}", a, [plain], [got])
    sel = _sel(T, clips, H, W, split)
    xc = TO._frames_of(x, T, sel).reshape(len(sel), T, H, W, 64).transpose(0, 2, 3, 1, 4).reshape(len(sel), H, W, 64 * T)
    ref = pfnl_spec.lrelu(pfnl_spec.conv2d_same(xc.astype(np.float64), k.astype(np.float64), b.astype(np.float64)))
    g_ = got.cpu().numpy()
    assert _rel(g_[sel][..., :cout], ref) < TO.SPLIT16_OP_REL_TOL
    assert not g_[..., cout:].any()


@pytest.mark.parametrize("mfma", [16, 32])
@pytest.mark.parametrize("g", GEOMS + SPLITS, ids=_gid)
def test_conv3x3_bf16_in_arena(g, mfma):
    """pfnl_op_conv3x3_bf16_ex (the fused mode of conv_bf16_v3.hip, both MFMA shapes, whole and cut chains): bf16 operands in a bf16-NaN flood."""
    T, clips, H, W, split = _geometry(g)
    x, addend, resid, k, b = TB._mode1_case(clips, T, H, W, seed=T + H + mfma)
    x16, a16, r16 = (v.to(torch.bfloat16) for v in (x, addend, resid))
    plain = ops.conv3x3_bf16_ex(x16.cuda(), k, b, a16.cuda(), T, r16.cuda(), mfma=mfma, split=split)
    a = _arena_of({"x": x16, "addend": a16, "resid": r16}, {"out": x.shape}, "bfloat16", H * W * 64)
    got = ops.conv3x3_bf16_ex(a["x"], k, b, a["addend"], T, a["resid"], mfma=mfma, split=split, out=a["out"])
    _arena_verdict(f"conv3x3_bf16_ex mfma={mfma} {_gid(g)}", a, [plain], [got])
    sel = _sel(T, clips, H, W, split)
    TB.close_bf16(TB._clips_of(got, T, sel), TB.ref_conv3(TB._clips_of(x, T, sel), k, b, True, addend[sel], T, TB._clips_of(resid, T, sel)))


@pytest.mark.parametrize("mfma", [16, 32])
@pytest.mark.parametrize("g", GEOMS + SPLITS, ids=_gid)
def test_conv1_conv10_bf16_in_arena(g, mfma):
    """pfnl_op_conv1_conv10_bf16_ex (conv1_i + conv10_i in one launch of conv_bf16_v3.hip; cut chains + c10_finalize_bf16_kernel)."""
    T, clips, H, W, split = _geometry(g)
    x, k1, b1, k10, b10 = TB._mode2_case(clips, T, H, W, seed=T * 3 + H + mfma)
    x16 = x.to(torch.bfloat16)
    plain = ops.conv1_conv10_bf16_ex(x16.cuda(), k1, b1, k10, b10, T, mfma=mfma, split=split)
    a = _arena_of({"x": x16}, {"out1": x.shape, "base": (clips, H, W, 64)}, "bfloat16", H * W * 64)
    got = ops.conv1_conv10_bf16_ex(a["x"], k1, b1, k10, b10, T, mfma=mfma, split=split, out1=a["out1"], base=a["base"])
    _arena_verdict(f"conv1_conv10_bf16_ex mfma={mfma} {_gid(g)}", a, plain, got)
    sel = _sel(T, clips, H, W, split)
    o1 = TB._clips_of(got[0].cpu(), T, sel)
    TB.close_bf16(o1, TB.ref_conv3(TB._clips_of(x, T, sel), k1, b1, True))
    TB.close_bf16(got[1].cpu()[sel], TB._base_ref(o1, k10, b10, T))


@pytest.mark.parametrize("name", [t.name for t in Hy.family_targets()])
def test_forward_device_in_arena(name):
    """PFNLEngine.forward_device with `in` and `out` in one arena (gaps of one LR clip frame's output, 16 x the LR frame): the nl pack and
    the tail's bicubic base read `in`, the tail writes `out`.  Same bits as on ordinary tensors (inside the oracle's bound); gaps intact."""
    t = Hy.target(name)
    x, xd, _ = _case(t)
    B, H, W = _shape(t)
    eng = _engine(t)
    y0 = Hy.run_device(eng, xd)
    verdict = _judge(t, y0)
    a = Hy.Arena({"in": (x.shape, "float32", x), "out": (eng.out_shape(B, H, W), "float32", None)}, 16 * H * W * 3 * 4)
    eng.forward_device(a["in"].data_ptr(), a["out"].data_ptr(), B, H, W)
    torch.cuda.synchronize()
    r = a.check()
    same = _same_bits(y0, a["out"].cpu().numpy())
    _report(t, "forward_device-arena", "identical" if same else "DIFFERENT", f"{verdict}; {r}")
    assert r.ok, str(r)
    assert same
    eng.close()
