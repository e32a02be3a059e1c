"""Distinct handles are independent from distinct host threads too (include/pfnl_hip.h; DESIGN.md "What handles share"; the harness and its
host tests: tests/threads.py, tests/test_threads_host.py).

Every test: at most four worker threads, each with an engine and a torch.cuda.Stream() of its own on device 0; all inputs prepared and all
reference results computed SERIALLY before the threads start - and held to the existing bounds against the oracle, so that "equally wrong
alone and together" cannot pass; then six rounds of all workers at once, every result compared BIT FOR BIT with its serial one.  The time
limit is max(60 s, 50 x the serial pass): a hang guard.  Every test prints its overlap share (pytest -s) and FAILS below one half.

A. device-pointer forwards, every pair of the six trunk families (three groups of four)
B. host-pointer forwards: the Python pinned pool, every handle's copy threads, one handle that reruns every call on the f32-MFMA kernels
C. two threads capture graphs (one of them on its handle's own blocking stream) while a third grows its workspace (hipFree + hipMalloc)
   and a fourth runs op hooks (hipMalloc, a blocking hipMemcpy through the null stream, hipFree)
D. two streaming sessions (rgb24; nv12 -> p010 at another size with the cut detector) and a forward
E. the cold start: the first library calls of a fresh process are four threads at once (tests/threads_cold.py)"""
import gc
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import history as Hy  # noqa: E402
import session_model as M  # noqa: E402   (the nv12 -> p010 session of part D against the host model)
import test_gpu_forward as TF  # noqa: E402   (ABS_TOL, _rel_err)
import test_gpu_history as GH  # noqa: E402   (_judge, _shape, _weights, _engine, _case, _geom, _same_bits)
import test_gpu_ops as TO  # noqa: E402   (SPLIT16_OP_REL_TOL, RESAMPLE_ABS_TOL)
import test_gpu_stream as TS  # noqa: E402   (_stream_all, _explicit, _frames_u8)
import threads as Th  # noqa: E402
import threads_cold as Cold  # noqa: E402
from oracle import pfnl_fast, pfnl_spec  # noqa: E402
from pfnl_amd import engine as E  # noqa: E402
from pfnl_amd import ops, synth, yuv  # noqa: E402
from pfnl_amd.engine import PFNLEngine  # noqa: E402


def _family(fam):
    return next(t for t in Hy.family_targets() if t.family == fam)


def _reachable(fam):
    """The family's target, or None - reported by name - where no shape under the cap reaches its structure on this device
    (test_gpu_history._shape's rule and message)."""
    t = _family(fam)
    try:
        GH._shape(t)
    except pytest.skip.Exception as e:
        print(f"\n[threads] left out by name: {e}", end="")
        return None
    return t


def _forward_worker(eng, xd, S):
    """A device-pointer forward on the worker's stream, that stream synchronised, then sync(): (bits, range flag).  xd: one device tensor, or
    one per round."""
    def work(r):
        x = xd[r] if isinstance(xd, (list, tuple)) else xd
        with torch.cuda.stream(S):
            y = eng.forward(x)
            S.synchronize()
            eng.sync()                                                            # (raises PFNL_ERR_RANGE for a flagged forward)
            return y.cpu().numpy(), eng.range_flagged()
    return work


def _engine_of(geom, w, **options):
    e = PFNLEngine(geom, device=0)
    e.load_weights(w)
    for k, v in options.items():
        e.set_option(k, v)
    return e


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


# ---- A. device-pointer forwards, every pair of trunk families ----------------------------------------------------------------------------

@pytest.mark.parametrize("group", Th.GROUPS_A, ids="-".join)
def test_device_forwards_of_every_family_pair(group):
    """Four families at once, each on its own engine and stream at the shape pfnl_plan gives it on this device: in every round no error, no
    range flag, and the bits of the worker's serial y0 (itself inside the forward tests' bound against the oracle)."""
    targets = [t for t in map(_reachable, group) if t is not None]
    if len(targets) < 2:
        pytest.skip(f"fewer than two families of {group} are in reach on this device")
    workers, engines = {}, []
    for t in targets:
        _, xd, _ = GH._case(t)
        engines.append(GH._engine(t))
        workers[t.family] = _forward_worker(engines[-1], xd, torch.cuda.Stream())
    serial, serial_s = Th.timed(lambda: {fam: w(0) for fam, w in workers.items()})
    verdicts = []
    for t in targets:
        y0, flagged = serial[t.family]
        assert not flagged, t.name
        verdicts.append(f"{t.family}: {GH._judge(t, y0)}")
    run = Th.run_together(workers, Th.ROUNDS, Th.hang_guard_s(serial_s))
    for t in targets:
        for r, (y, flagged) in enumerate(run.results[t.family]):
            assert not flagged, (t.name, r)
            assert GH._same_bits(serial[t.family][0], y), (t.name, r, int((serial[t.family][0] != y).sum()))
    Th.require_overlap("A " + "-".join(group), run, serial_s, "; ".join(verdicts))
    for e in engines:
        e.close()


# ---- B. host-pointer forwards -------------------------------------------------------------------------------------------------------------

HOST_SHAPE = (1, 7, 64, 64)                       # the result, 768 KiB, comes from engine._pinned_pool (from 512 KiB)
POOL_SHAPE = (2, 7, 64, 64)                       # a pageable INPUT of 672 KiB: staged by the handle's copy threads (capi.hip STAGE_POOL_MIN, 512 KiB)


def _host_worker(eng, x, as_torch):
    def work(r):
        y = eng.forward(torch.from_numpy(x) if as_torch else x)
        return (y.numpy() if as_torch else y), eng.range_reruns()
    return work


def test_host_forwards_share_the_pinned_pool(monkeypatch):
    """numpy in -> numpy out on three handles at 1 x 7 x 64 x 64 - one plain, one through a torch CPU tensor, one with the overflow weights
    of test_split16_domain_activation_overflow_is_caught, whose every call is flagged and redone on the f32-MFMA kernels - and a fourth at
    two clips, whose pageable input is large enough for the handle's copy-thread pool (a pinned result bypasses the pool, and one clip's input
    is below its threshold).  Per round: the serial bits; one more rerun for the flagged handle and none for the others; no two results
    alive at the same time share memory.  Afterwards the pool's books are in order and within its cap."""
    monkeypatch.delenv("PFNL_HOST_OUTPUT", raising=False)
    t = _family("small")
    geom, w = GH._geom(t), GH._weights(t)
    w_over = synth.synthetic_weights(geom, seed=1)
    w_over["nlvsr/conv0/kernel"] = (w_over["nlvsr/conv0/kernel"] * 4e5).astype(np.float32)
    cases = {"numpy": (w, HOST_SHAPE, 21, False), "torch-cpu": (w, HOST_SHAPE, 22, True), "overflow": (w_over, HOST_SHAPE, 3, False),
             "two-clips": (w, POOL_SHAPE, 24, False)}
    assert int(np.prod(POOL_SHAPE)) * 3 * 4 >= 512 << 10 > int(np.prod(HOST_SHAPE)) * 3 * 4
    workers, engines, refs = {}, [], {}
    for name, (wt, shape, seed, as_torch) in cases.items():
        x = synth.uniform_clips(*shape, seed=seed)
        refs[name] = pfnl_fast.FastOracle(wt, t.T, 4, GH.NB).forward(x)
        engines.append(_engine_of(geom, wt))
        workers[name] = _host_worker(engines[-1], x, as_torch)
    serial, serial_s = Th.timed(lambda: {name: wk(0) for name, wk in workers.items()})
    for name, (y0, reruns) in serial.items():
        assert y0.nbytes >= 512 << 10 and not y0.flags.owndata, name            # a view of a pool block, not numpy's own memory
        assert np.isfinite(y0).all() and reruns == (1 if name == "overflow" else 0), (name, reruns)
        if name == "overflow":
            assert TF._rel_err(y0, refs[name]) < 5e-5, TF._rel_err(y0, refs[name])
        else:
            assert float(np.abs(y0 - refs[name]).max()) < TF.ABS_TOL, name
    run = Th.run_together(workers, Th.ROUNDS, Th.hang_guard_s(serial_s))
    alive = [(name, -1, serial[name][0]) for name in workers]
    for name in workers:
        for r, (y, reruns) in enumerate(run.results[name]):
            assert GH._same_bits(serial[name][0], y), (name, r, int((serial[name][0] != y).sum()))
            assert reruns == (serial[name][1] + r + 1 if name == "overflow" else 0), (name, r, reruns)
            alive.append((name, r, y))
    assert len({a.ctypes.data for _, _, a in alive}) == len(alive)
    for i, (n1, r1, a) in enumerate(alive):
        for n2, r2, b in alive[i + 1:]:
            assert not np.shares_memory(a, b), (n1, r1, n2, r2)
    Th.require_overlap("B host pointers", run, serial_s, f"{len(alive)} results alive, pool holds {E._pinned_pool.free_bytes() >> 10} KiB")
    del alive, run, serial, y0, y, a, b
    gc.collect()
    pool = E._pinned_pool
    assert pool.free_bytes() == sum(n * len(blocks) for n, blocks in pool._free.items())
    assert 0 < pool.free_bytes() <= pool._cap(), (pool.free_bytes(), pool._cap())
    ptrs = [p for blocks in pool._free.values() for p in blocks]
    assert len(set(ptrs)) == len(ptrs)                                            # no block was given back twice
    for e in engines:
        e.close()


# ---- C. capture beside allocation and null-stream copies ----------------------------------------------------------------------------------

OPS_PER_ROUND = 4


def _ops_case():
    rng = np.random.default_rng(357)
    T, H, W, cout = 3, 5, 7, 48
    x = rng.normal(size=(T, H, W, 64)).astype(np.float32)
    k = (rng.normal(size=(3, 3, 64 * T, cout)) / np.sqrt(576 * T)).astype(np.float32)
    b = (rng.normal(size=cout) * 0.1).astype(np.float32)
    lr = rng.random((2, 16, 24, 3), dtype=np.float32)
    xc = x.reshape(1, T, H, W, 64).transpose(0, 2, 3, 1, 4).reshape(1, H, W, 64 * T)
    ref_conv = pfnl_spec.lrelu(pfnl_spec.conv2d_same(xc.astype(np.float64), k.astype(np.float64), b.astype(np.float64)))
    ref_bic = pfnl_spec.resize_bicubic_tf1(lr.astype(np.float64), 4)
    return x, k, b, lr, T, ref_conv, ref_bic


def test_capture_beside_allocation_and_null_stream_copies():
    """graph=on on two handles, a new small shape per round and three calls per shape - eager, capture, replay - all three equal to the
    serial graph=off result: one handle on a stream of the worker's, one with stream = NULL, where the capture runs on the handle's own
    BLOCKING stream (hipStreamCaptureModeThreadLocal).  Beside them a handle whose shape grows every round (DevBuf::ensure: hipFree +
    hipMalloc, and a bump of the process-wide g_alloc_gen that makes the other two capture again) and a thread of op hooks with host
    weights (OpStage: hipMalloc, a blocking hipMemcpy through the legacy null stream, hipFree).  The runtime refuses such a copy while any
    thread's capture is open and invalidates the capture (HIP 7.2; DESIGN.md "What handles share"): the library keeps the two apart with
    one process-wide lock (common.h CaptureGuard / BlockingCopyGuard).  Without it this test fails whenever the two coincide - rarely."""
    t = _family("small")
    geom, w = GH._geom(t), GH._weights(t)
    oracle = pfnl_fast.FastOracle(w, t.T, 4, GH.NB)
    shapes = {"graph-own-stream": [(1, 8 + 2 * r, 16) for r in range(Th.ROUNDS)],
              "graph-null-stream": [(1, 10 + 2 * r, 12) for r in range(Th.ROUNDS)],
              "growing": [(1, 16 + 8 * r, 24 + 8 * r) for r in range(Th.ROUNDS)]}
    xs = {n: [synth.uniform_clips(B, t.T, H, W, seed=40 + 7 * i + r) for r, (B, H, W) in enumerate(s)] for i, (n, s) in enumerate(shapes.items())}
    xd = {n: [torch.from_numpy(x).cuda() for x in v] for n, v in xs.items()}
    refs = {n: [oracle.forward(x) for x in v] for n, v in xs.items()}
    x3, k3, b3, lr, T3, ref_conv, ref_bic = _ops_case()
    x3d, lrd = torch.from_numpy(x3).cuda(), torch.from_numpy(lr).cuda()
    S_ops = torch.cuda.Stream()

    def ops_once():
        with torch.cuda.stream(S_ops):
            a = ops.conv3x3_accum(x3d, k3, b3, act=True, frames_per_clip=T3, variant="split16")
            c = ops.bicubic(lrd, 4)
            S_ops.synchronize()
            return a.cpu().numpy(), c.cpu().numpy()

    def serial_pass():
        ref_eng = _engine_of(geom, w, graph="off")
        y0 = {n: [Hy.run_device(ref_eng, x) for x in v] for n, v in xd.items()}
        ref_eng.close()
        return y0, ops_once()

    (y0, (conv0, bic0)), serial_s = Th.timed(serial_pass)
    worst = max(float(np.abs(y - ref).max()) for n in y0 for y, ref in zip(y0[n], refs[n]))
    assert all(np.isfinite(y).all() for v in y0.values() for y in v) and worst < TF.ABS_TOL, worst
    e_conv = float(np.abs(conv0 - ref_conv).max() / max(1.0, np.abs(ref_conv).max()))
    assert e_conv < TO.SPLIT16_OP_REL_TOL and float(np.abs(bic0 - ref_bic).max()) < TO.RESAMPLE_ABS_TOL, e_conv

    engines = {n: _engine_of(geom, w, graph="off" if n == "growing" else "on") for n in shapes}     # new handles: nothing allocated yet
    S_own = torch.cuda.Stream()
    outs = [torch.empty(engines["graph-null-stream"].out_shape(*s), dtype=torch.float32, device="cuda") for s in shapes["graph-null-stream"]]

    def graph_own_stream(r):
        eng, ys = engines["graph-own-stream"], []
        with torch.cuda.stream(S_own):
            for _ in range(3):
                y = eng.forward(xd["graph-own-stream"][r])
                S_own.synchronize()
                ys.append(y.cpu().numpy())
            eng.sync()
        return ys

    def graph_null_stream(r):
        eng, ys = engines["graph-null-stream"], []
        B, H, W = shapes["graph-null-stream"][r]
        for _ in range(3):
            outs[r].fill_(float("nan"))                                           # (on the null stream, as the call itself)
            eng.forward_device(xd["graph-null-stream"][r].data_ptr(), outs[r].data_ptr(), B, H, W)   # stream = NULL
            eng.sync()
            ys.append(outs[r].cpu().numpy())
        return ys

    workers = {"graph-own-stream": graph_own_stream, "graph-null-stream": graph_null_stream,
               "growing": _forward_worker(engines["growing"], xd["growing"], torch.cuda.Stream()),
               "ops": lambda r: [ops_once() for _ in range(OPS_PER_ROUND)]}
    torch.cuda.synchronize()
    run = Th.run_together(workers, Th.ROUNDS, Th.hang_guard_s(serial_s))
    for n in ("graph-own-stream", "graph-null-stream"):
        for r, ys in enumerate(run.results[n]):
            same = [GH._same_bits(y0[n][r], y) for y in ys]
            assert all(same), (n, r, shapes[n][r], same)                          # eager, capture, replay
    for r, (y, flagged) in enumerate(run.results["growing"]):
        assert not flagged and GH._same_bits(y0["growing"][r], y), ("growing", r, shapes["growing"][r])
    for r, res in enumerate(run.results["ops"]):
        for a, c in res:
            assert _same(a, conv0) and _same(c, bic0), ("ops", r)
    Th.require_overlap("C capture + allocation + null stream", run, serial_s, f"worst serial error {worst:.2g}")
    for e in engines.values():
        e.close()


# ---- D. two sessions and a forward ---------------------------------------------------------------------------------------------------------

FRAMES = 10


def _two_scenes():
    """FRAMES RGB frames of 16 x 24 with a real cut in the middle: one random image per scene and noise of +-2 a frame, as
    session_model.content makes its scenes."""
    rng = np.random.default_rng(9)
    out = []
    for _ in range(2):
        base = rng.integers(0, 256, size=(M.H, M.W, 3))
        out += [np.clip(base + rng.integers(-2, 3, size=base.shape), 0, 255).astype(np.uint8) for _ in range(FRAMES // 2)]
    return out


def _drive(vs, frames):
    """One sequence through an open session on host pointers: (indices, frames, cuts); the session is left reset for the next one."""
    got = TS._stream_all(vs, frames)
    cuts = list(vs.cuts)
    vs.reset()
    return [i for i, _ in got], [f for _, f in got], cuts


def _same_sequence(got, want):
    return got[0] == want[0] and got[2] == want[2] and len(got[1]) == len(want[1]) and all(_same(a, b) for a, b in zip(got[1], want[1]))


def test_two_sessions_and_a_forward():
    """A default rgb24 session, an nv12 session that delivers p010 at 48 x 72 with the cut detector on (the edge kernels, the resampler's
    tables, the scene kernel's scratch counters) and a plain forward on a handle without a session.  Ten frames of 16 x 24 pushed and
    popped per round on host pointers: the bytes and cuts of the same session driven alone - which are those of the explicit path (rgb24)
    and of the host model around the plain session (session_model.expected)."""
    t = _family("small")
    geom, w = GH._geom(t), GH._weights(t)
    row = M.with_(M.DEFAULT, in_=("nv12", 8, "420", None), out=("p010", "420", None), scenes="detector", size="shrink", batch=2)
    assert M.legal(row) and (M.H, M.W) == (16, 24)
    rgb_frames = list(TS._frames_u8(FRAMES, M.H, M.W, seed=71))
    nv12_frames = [np.ascontiguousarray(yuv.from_rgb(f, "nv12")) for f in _two_scenes()]
    e_rgb, e_nv12, e_base = (_engine_of(geom, w) for _ in range(3))

    def base(brow, frames, marks):
        assert brow.out[0] == "rgb10" and brow.scenes == "detector" and not marks
        with e_base.open_stream(M.H, M.W, batch=brow.batch, scene_cut=M.THRESHOLD, out_format="rgb10") as vs:
            got = TS._stream_all(vs, [np.ascontiguousarray(f) for f in frames])
            base.cuts = list(vs.cuts)
        return [f for _, f in got]

    want_nv12 = M.expected(row, nv12_frames, base)
    assert base.cuts == [FRAMES // 2], base.cuts                                   # the cut the content holds
    want_rgb = TS._explicit(e_base, np.stack(rgb_frames), 2, geom.num_frames)
    e_base.close()

    S1, S2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(S1):
        vs_rgb = e_rgb.open_stream(M.H, M.W, batch=2)
    with torch.cuda.stream(S2):
        vs_nv12 = e_nv12.open_stream(M.H, M.W, batch=2, scene_cut=M.THRESHOLD, pixel_format="nv12", out_format="p010",
                                     out_size=M.SIZES["shrink"]["out_size"])
    ft = _family("small")
    e_fwd = GH._engine(ft)
    workers = {"rgb24": lambda r: _drive(vs_rgb, rgb_frames), "nv12-p010": lambda r: _drive(vs_nv12, nv12_frames),
               "forward": _forward_worker(e_fwd, GH._case(ft)[1], torch.cuda.Stream())}
    serial, serial_s = Th.timed(lambda: {n: wk(0) for n, wk in workers.items()})
    assert serial["rgb24"][0] == list(range(FRAMES)) and serial["rgb24"][2] == []
    assert _same(np.stack(serial["rgb24"][1]), want_rgb)
    assert _same_sequence(serial["nv12-p010"], ([i for i, _ in want_nv12], [f for _, f in want_nv12], base.cuts))
    verdict = GH._judge(ft, serial["forward"][0])
    assert not serial["forward"][1]
    run = Th.run_together(workers, Th.ROUNDS, Th.hang_guard_s(serial_s))
    for n in ("rgb24", "nv12-p010"):
        for r, got in enumerate(run.results[n]):
            assert _same_sequence(got, serial[n]), (n, r, got[0], got[2])
    for r, (y, flagged) in enumerate(run.results["forward"]):
        assert not flagged and GH._same_bits(serial["forward"][0], y), ("forward", r)
    Th.require_overlap("D two sessions and a forward", run, serial_s, f"forward {verdict}; cuts {base.cuts}")
    vs_rgb.close()
    vs_nv12.close()
    for e in (e_rgb, e_nv12, e_fwd):
        e.close()


# ---- E. cold start --------------------------------------------------------------------------------------------------------------------------

def test_cold_start_of_four_threads_in_a_fresh_process(tmp_path):
    """tests/threads_cold.py in a child process (a fresh one, started once; two processes hold the device): small, chain, bf16 and a
    blur_decimate + bicubic worker are the first library calls of that process, at once and without a warm-up.  Their bits are this
    process's serial ones.  A nonzero exit, the time limit or a missing file fails the test."""
    targets = {fam: t for fam, t in ((fam, _reachable(fam)) for fam in Cold.FAMILIES) if t is not None}
    shapes = {fam: GH._shape(t) for fam, t in targets.items()}
    hr, lr = Cold.op_inputs()
    engines = {fam: GH._engine(t) for fam, t in targets.items()}
    for fam, t in targets.items():
        assert _same(Cold.clip(t, shapes[fam]), GH._case(t)[0]) and all(_same(v, Cold.weights(t)[k]) for k, v in GH._weights(t).items())

    def serial_pass():
        y0 = {fam: Hy.run_device(engines[fam], GH._case(t)[1]) for fam, t in targets.items()}
        blur = ops.blur_decimate(torch.from_numpy(hr).cuda(), Cold.SCALE).cpu().numpy()
        bic = ops.bicubic(torch.from_numpy(lr).cuda(), Cold.SCALE).cpu().numpy()
        return y0, blur, bic

    (y0, blur0, bic0), serial_s = Th.timed(serial_pass)
    verdicts = [f"{fam}: {GH._judge(t, y0[fam])}" for fam, t in targets.items()]
    assert float(np.abs(blur0 - synth.blur_decimate(hr.astype(np.float64), Cold.SCALE)).max()) < TO.RESAMPLE_ABS_TOL
    assert float(np.abs(bic0 - pfnl_spec.resize_bicubic_tf1(lr.astype(np.float64), Cold.SCALE)).max()) < TO.RESAMPLE_ABS_TOL
    for e in engines.values():
        e.close()

    shapes_path, out_path = str(tmp_path / "shapes.json"), str(tmp_path / "cold.npz")
    with open(shapes_path, "w") as f:
        json.dump({fam: list(s) for fam, s in shapes.items()}, f)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(Cold.__file__), shapes_path, out_path]
    p = subprocess.run(cmd, timeout=Th.hang_guard_s(serial_s) + Cold.CHILD_TIMEOUT_S, capture_output=True, text=True)
    assert p.returncode == 0, (p.returncode, p.stdout[-1000:], p.stderr[-3000:])
    assert os.path.exists(out_path), "the child left no result file"
    got = np.load(out_path)
    for fam, t in targets.items():
        assert str(got["structure_" + fam]) == t.structure, (fam, str(got["structure_" + fam]))
        assert GH._same_bits(y0[fam], got["y_" + fam]), (fam, int((y0[fam] != got["y_" + fam]).sum()))
    assert _same(blur0, got["blur"]) and _same(bic0, got["bicubic"])
    names = list(targets) + ["ops"]
    stamps = {n: [tuple(got["stamps_" + n])] for n in names}
    run = Th.Run(names, {n: [None] for n in names}, stamps, wall_s=max(b for v in stamps.values() for _, b in v) - min(a for v in stamps.values() for a, _ in v))
    Th.require_overlap("E cold start in a child process", run, serial_s, "; ".join(verdicts))
