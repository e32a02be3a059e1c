"""The stream contract on non-blocking streams (include/pfnl_hip.h STREAMS; DESIGN.md "What a call is ordered with"; helpers:
tests/streams.py).  The other GPU tests run on the legacy null stream, which synchronises implicitly with the handle's blocking stream:
a launch on the wrong stream, a missing event or a step parked on the handle's stream is invisible there.  Here every call runs on a
hipStreamNonBlocking stream S behind a delay that makes a mis-ordered step read a NaN / 0xA5 fill (Probe L), or while the null stream
spins (Probe N: right bits, and e0 behind the spin still pending - the call neither ran on nor waited for the null stream).

A. the two controls: the probes discriminate on this device (else every probe FAILS as insensitive).
B. PFNLEngine.forward of a device tensor: one target per trunk family + the general non-local family + T = 3, at graph=off (the default);
   the graph path: eager, capture + replay, replay with three different inputs, then an option change and back (drop, recapture).
C. forward_strip: two strips that tile a frame.            D. an engine and its clone on two streams, both in flight.
E. the streaming session opened on S: device frames, every edge kernel, mixed device / host pushes with scenes, host frames, the scene
   table's setup, the range rerun, a plain forward between pushes, reset with a batch in flight.
F. the asynchronous op hooks.   G. three host-synchronising hooks (Probe L only).   H. the range flag of an asynchronous call.

References: the same scenario on the default stream on a fresh engine, no delays; a forward's reference also passes the bound of the
existing forward test of its precision.  Every case prints one line (pytest -s): scenario, probe, D, verdict."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import history as Hy  # noqa: E402
import streams as St  # noqa: E402
import test_gpu_depth10 as TD  # noqa: E402   (the 10-bit frames of the op tests)
import test_gpu_forward as TF  # noqa: E402   (ABS_TOL)
import test_gpu_history as TH  # noqa: E402   (the targets' shapes, engines, cases and _judge)
import test_gpu_ops as TO  # noqa: E402   (the split geometries, the chain launch's fp64 reference, SPLIT16_OP_REL_TOL)
import test_gpu_scene as TSC  # noqa: E402   (the content with cuts)
import test_gpu_score as TSY  # noqa: E402   (content pairs, the comparison with pfnl_amd.metrics)
import test_gpu_stream as TS  # noqa: E402   (frames, the session's range-rerun weights)
import test_gpu_yuv as TY  # noqa: E402   (packed 4:2:0 frames)
from oracle import pfnl_fast, pfnl_spec  # noqa: E402
from pfnl_amd import depth10, ops, scene, synth, yuv  # noqa: E402
from pfnl_amd import model as M  # noqa: E402
from pfnl_amd.spec import PFNLGeometry  # noqa: E402

PUSH_D_MS = 5.0                                  # Probe L inside a session: the spin in front of every late frame copy
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _streams_teardown():
    import gc
    gc.collect()                                  # handles and sessions that earlier modules dropped without closing hold streams
    yield
    St.teardown()


def _verdict(p, probe, refs, extra=""):
    """warm-up, the probe, one line, the assertions: bits equal to `refs` (and e0 pending for Probe N)."""
    warm = p.warm_up()
    if probe == "L":
        got, pending = p.late(), None
    else:
        got, pending = p.null_asleep()
    same = len(got) == len(refs) and all(St.same_bits(g, r) for g, r in zip(got, refs))
    bad = "" if same else "DIFFERENT: " + ", ".join("%d of %d bytes" % (int((np.ascontiguousarray(g).reshape(-1).view(np.uint8) != np.ascontiguousarray(
        r).reshape(-1).view(np.uint8)).sum()), r.nbytes) if g.nbytes == r.nbytes else "another size" for g, r in zip(got, refs))
    St.report(p.label, "probe " + probe, p.D, ("identical" if same else bad) + ("" if pending is None else ", e0 pending" if pending else ", e0 DONE"), extra)
    assert all(St.same_bits(g, r) for g, r in zip(warm, refs)), f"{p.label}: the undelayed run on the side stream differs from the default stream's"
    assert same, f"{p.label}: probe {probe} {bad}"
    if pending is not None:
        assert pending, f"{p.label}: the call ran on, or waited for, the null stream (or the handle's blocking stream behind it)"


# ---- A. the controls -----------------------------------------------------------------------------------------------------------------

def test_control_late_input_is_seen_by_an_unordered_copy():
    """Control L at the smallest D a probe can get: an unordered plain copy issued on the null stream, and one issued on the second side
    stream, see the fill."""
    sens = St.sensitivity()
    St.report("control L (null stream; second side stream)", "control", St.CONTROL_D_MS, f"{sens['L']}; {sens['pair']}", sens["how"])
    assert sens["L"], f"insensitive on this device: {sens['how']}"
    assert sens["L2"] and sens["pair"], f"insensitive on this device (second side stream): {sens['how']}"
    assert St.control_late(St.side_stream(), D=PUSH_D_MS), "insensitive on this device at the sessions' per-push delay"


def test_control_side_stream_runs_while_the_null_stream_sleeps():
    """Control N: a plain torch op on S completes and S.synchronize() returns while the event behind the null stream's spin is pending."""
    sens = St.sensitivity()
    St.report("control N", "control", St.CONTROL_D_MS, str(sens["N"]), sens["how"])
    assert sens["N"], f"insensitive on this device: {sens['how']}"


# ---- B. forward --------------------------------------------------------------------------------------------------------------------

FORWARD_TARGETS = [t.name for t in Hy.family_targets()] + ["nl_sub_sample2", "nl_type0", "T3-chain2_split"]
SMALL = Hy.family_targets()[0].name


def _forward_ref(t):
    """The target's clip and its result on a fresh engine on the default stream, inside the existing forward test's bound."""
    key = ("fwd", t.name)
    if key not in _cache:
        x, xd, _ = TH._case(t)
        eng = TH._engine(t)
        y0 = Hy.run_device(eng, xd)
        eng.close()
        _cache[key] = (x, y0, TH._judge(t, y0))
    return _cache[key]


@pytest.mark.parametrize("probe", ["L", "N"])
@pytest.mark.parametrize("name", FORWARD_TARGETS)
def test_forward_on_a_side_stream(name, probe):
    """pfnl_forward with device pointers on S, graph=off (the eager path: every launch of forward_device takes the caller's stream)."""
    t = Hy.target(name)
    x, y0, bound = _forward_ref(t)
    S = St.side_stream()
    eng = TH._engine(t)
    try:
        assert eng.get_option("graph") == "off"
        _verdict(St.Probe(f"forward {name} {t.structure} {'x'.join(map(str, x.shape[:4]))}", S, [x], lambda b: [eng.forward(b[0])]), probe, [y0], bound)
        assert eng.range_flagged() is False
    finally:
        eng.close()


def _small_inputs():
    """Three clips at the small target's shape with their oracle results."""
    if "small_inputs" not in _cache:
        t = Hy.target(SMALL)
        B, H, W = TH._shape(t)
        xs = [synth.uniform_clips(B, t.T, H, W, seed=500 + i) for i in range(3)]
        orc = pfnl_fast.FastOracle(TH._weights(t), t.T, 4, TH.NB)
        _cache["small_inputs"] = (xs, [orc.forward(x) for x in xs])
    return _cache["small_inputs"]


GRAPH_CALLS = [(0, "eager"), (1, "capture+replay"), (2, "replay"), (0, "drop, eager"), (1, "recapture+replay")]   # (input, what the call is)


def _graph_sequence(eng, call):
    """graph=auto: three calls; conv3x3=direct and back (the captured graph is stale); two more.  call(k, input index) -> result."""
    back = eng.get_option("conv3x3")
    eng.set_option("graph", "auto")
    ys = [call(k, GRAPH_CALLS[k][0]) for k in range(3)]
    eng.set_option("conv3x3", "direct")
    eng.set_option("conv3x3", back)
    return ys + [call(k, GRAPH_CALLS[k][0]) for k in (3, 4)]


def _graph_ref():
    if "graph_ref" not in _cache:
        t = Hy.target(SMALL)
        xs, orcs = _small_inputs()
        xd = [torch.from_numpy(x).cuda() for x in xs]
        eng = TH._engine(t)
        ys = _graph_sequence(eng, lambda k, i: Hy.run_device(eng, xd[i]))
        eng.close()
        for (i, what), y in zip(GRAPH_CALLS, ys):
            err = float(np.abs(y - orcs[i]).max())
            assert np.isfinite(y).all() and err < TF.ABS_TOL, (what, err)
        _cache["graph_ref"] = ys
    return _cache["graph_ref"]


@pytest.mark.parametrize("probe", ["L", "N"])
def test_forward_graph_path_on_a_side_stream(probe):
    """The graph path of pfnl_forward on S (capture happens on the caller's stream; the staging copies and hipGraphLaunch go there): the
    eager call, the capture + replay and a replay, each with ANOTHER input (a kernel left out of the capture would replay nothing new)
    and each against its own reference; then an option change and back - the stale graph is dropped, the shape recaptured on S.
    The warm-up runs at graph=off, plus one host-pointer forward that allocates the staging buffers: no graph exists when the probed calls begin."""
    t = Hy.target(SMALL)
    xs, _ = _small_inputs()
    refs = _graph_ref()
    S = St.side_stream()
    eng = TH._engine(t)
    try:
        body = lambda b: [eng.forward(b[0])]                                     # noqa: E731
        probes = [St.Probe(f"forward {SMALL} graph=auto, input {i}", S, [x], body) for i, x in enumerate(xs)]
        warm = probes[0].warm_up()
        eng.forward(xs[0])
        for p in probes[1:]:
            p.D, p.host = probes[0].D, probes[0].host
        verdicts = []

        def call(k, i):
            if probe == "L":
                y, pending = probes[i].late()[0], None
            else:
                (y,), pending = probes[i].null_asleep()
            verdicts.append((GRAPH_CALLS[k][1], St.same_bits(y, refs[k]), pending))
            return y

        _graph_sequence(eng, call)
        for what, same, pending in verdicts:
            St.report(f"forward {SMALL} graph=auto: {what}", "probe " + probe, probes[0].D,
                      ("identical" if same else "DIFFERENT") + ("" if pending is None else ", e0 pending" if pending else ", e0 DONE"))
        assert St.same_bits(warm[0], _forward_graph_off_ref(0))
        assert all(same for _, same, _ in verdicts), verdicts
        assert all(pending is not False for _, _, pending in verdicts), verdicts
        assert eng.range_flagged() is False
    finally:
        eng.close()


def _forward_graph_off_ref(i):
    """The small target's eager result for input i: what every call of the graph sequence with that input returns as well."""
    refs = _graph_ref()
    return refs[[k for k, (j, _) in enumerate(GRAPH_CALLS) if j == i][0]]


def test_graph_replays_return_the_eager_bits():
    """The reference sequence itself: a replay returns what the eager call of the same input returns (inputs 0 and 1 occur twice)."""
    refs = _graph_ref()
    assert St.same_bits(refs[0], refs[3]) and St.same_bits(refs[1], refs[4])
    assert not St.same_bits(refs[0], refs[1]) and not St.same_bits(refs[1], refs[2])


# ---- C. forward_strip -----------------------------------------------------------------------------------------------------------------

def _strips(eng, x, out):
    H = x.shape[2]
    r = (H // 2) & ~1
    eng.forward_strip(x, out, 0, r)
    eng.forward_strip(x, out, r, H - r)
    return [out]


@pytest.mark.parametrize("probe", ["L", "N"])
def test_forward_strip_on_a_side_stream(probe):
    """Two strips tile one frame of the mid target; the union equals the default-stream union bit for bit (and the oracle at the forward's bound)."""
    t = Hy.family_targets()[1]
    x, xd, _ = TH._case(t)
    B, H, W = TH._shape(t)
    if "strip" not in _cache:
        eng = TH._engine(t)
        out = torch.full(eng.out_shape(B, H, W), float("nan"), dtype=torch.float32, device="cuda")
        _strips(eng, xd, out)
        torch.cuda.synchronize()
        y0 = out.cpu().numpy()
        eng.close()
        _cache["strip"] = (y0, TH._judge(t, y0))
    y0, bound = _cache["strip"]
    S = St.side_stream()
    eng = TH._engine(t)
    try:
        out = torch.empty(eng.out_shape(B, H, W), dtype=torch.float32, device="cuda")
        _verdict(St.Probe(f"forward_strip x 2 {t.name}", S, [x], lambda b: _strips(eng, b[0], out), owned=[out]), probe, [y0], bound)
    finally:
        eng.close()


# ---- D. two handles on two streams ---------------------------------------------------------------------------------------------------

def test_an_engine_and_its_clone_run_on_two_streams():
    """engine.clone's docstring: handles are independent, two of them on two streams keep two forwards in flight.  Probe L on each, on a
    side stream of its own, different inputs, both enqueued before either is synchronised; each result equals its serial reference."""
    St.require("L")
    St.require("L2")
    t = Hy.target(SMALL)
    xs, _ = _small_inputs()
    refs = [_forward_graph_off_ref(0), _forward_graph_off_ref(1)]
    eng = TH._engine(t)
    twin = eng.clone()
    try:
        pa = St.Probe("two handles: the engine", St.side_stream(), [xs[0]], lambda b: [eng.forward(b[0])])
        pb = St.Probe("two handles: its clone", St.side_stream(second=True), [xs[1]], lambda b: [twin.forward(b[0])], kind="L2")
        wa, wb = pa.warm_up(), pb.warm_up()
        pa.D = pb.D = max(pa.D, pb.D)
        pa.enqueue_late()
        pb.enqueue_late()
        ya, yb = pa.finish()[0], pb.finish()[0]
        for p, y, r in ((pa, ya, refs[0]), (pb, yb, refs[1])):
            St.report(p.label, "probe L", p.D, "identical" if St.same_bits(y, r) else "DIFFERENT")
        assert St.same_bits(wa[0], refs[0]) and St.same_bits(wb[0], refs[1])
        assert St.same_bits(ya, refs[0]) and St.same_bits(yb, refs[1])
    finally:
        twin.close()
        eng.close()


# ---- E. the session opened on S --------------------------------------------------------------------------------------------------------

GEOM1 = PFNLGeometry(num_block=1)
SH, SW, SBATCH = 16, 24, 3


def _engine1(w=None, precision="fp32"):
    return TS._engine_with(GEOM1, synth.synthetic_weights(GEOM1, seed=0) if w is None else w, precision)


class Frames:
    """The frames of one sequence: numpy, and for the device-pushed ones a device buffer (filled, or holding the frame) + a pinned copy."""

    def __init__(self, frames, device_mask):
        self.frames, self.mask = list(frames), list(device_mask)
        self.bufs = {k: St.to_device(f) for k, f in enumerate(self.frames) if self.mask[k]}
        self.pins = {k: St.pinned_like(self.frames[k]) for k in self.bufs}
        torch.cuda.synchronize()

    def prepare(self, real):
        for k, b in self.bufs.items():
            if real:
                St._as_int(b).copy_(self.pins[k])
            else:
                St.fill_pattern(b)
        torch.cuda.synchronize()


def _play(vs, fr, late_ms=None, marks=(), at=None, stop=None):
    """Pushes the frames (a device frame behind `late_ms` of spin and its late copy when late_ms is given), collecting what push and end
    return and every last_info; at = (k, fn): fn() in front of push k.  -> ([(index, frame)], [last_info])"""
    got, infos = [], []
    pop = vs.pop

    def pop_and_note():
        item = pop()
        if item is not None:
            infos.append(vs.last_info)
        return item

    vs.pop = pop_and_note
    try:
        for k, f in enumerate(fr.frames[:stop]):
            if at is not None and at[0] == k:
                at[1]()
            if k in marks:
                vs.mark_cut()
            if fr.mask[k]:
                if late_ms is not None:
                    St.sleep_ms(late_ms)
                    St._as_int(fr.bufs[k]).copy_(fr.pins[k], non_blocking=True)
                got += vs.push(fr.bufs[k])
            else:
                got += vs.push(f)
        if stop is None:
            got += vs.end()
    finally:
        del vs.pop
    return got, infos


def _host_frames(got):
    """After the stream has been synchronised: [(index, numpy frame)]"""
    return [(i, f if isinstance(f, np.ndarray) else St.to_numpy(St._as_int(f).cpu(), f)) for i, f in got]


def _session_reference(key, make_engine, open_kw, frames, mask, **play_kw):
    """The default-stream session on a fresh engine, no delays: (indices, frames stacked, infos, cuts)."""
    if key not in _cache:
        eng = make_engine()
        fr = Frames(frames, mask)
        with eng.open_stream(**open_kw) as vs:
            got, infos = _play(vs, fr, **play_kw)
            torch.cuda.synchronize()
            got = _host_frames(got)
            cuts = list(vs.cuts)
        eng.close()
        _cache[key] = ([i for i, _ in got], np.stack([f for _, f in got]), infos, cuts)
    return _cache[key]


def _session_probe(label, probe, eng, open_kw, frames, mask, ref, marks=()):
    """The session opened on S: an undelayed sequence (sets D for Probe N), reset, the probed sequence; frames, indices, infos and cuts
    against the reference.

    Probe N with host-pointer frames also needs the session's COPY stream off the null stream's hardware queue.  That stream is the
    library's own and its queue is the runtime's choice: a process with more live streams than hardware queues may put it next to the
    null stream, whose spin then delays every copy - a property of the placement, not of the session.  So the probe is taken on up to
    one placement per hardware queue: when the bits are right but e0 has completed, the session is closed, one more explicit stream is
    kept alive (the next copy stream lands on another queue) and the session reopened.  A session that waits for the null stream by
    its own doing does so on every queue and fails; each line says which placement it reports."""
    S = St.side_stream()
    St.require(probe)
    fr = Frames(frames, mask)
    idx, want, rinfos, rcuts = ref
    placements = St.MAX_EXPLICIT_TRIES if probe == "N" and not all(mask) else 1
    for attempt in range(placements):
        with torch.cuda.stream(S):
            vs = eng.open_stream(**open_kw)
        try:
            fr.prepare(real=True)
            t0 = time.perf_counter()
            with torch.cuda.stream(S):
                warm, winfos = _play(vs, fr, marks=marks)
            S.synchronize()
            D = St.delay_ms((time.perf_counter() - t0) * 1e3)
            warm = _host_frames(warm)
            wcuts = list(vs.cuts)
            vs.reset()
            pending, wall = None, None
            if probe == "L":
                fr.prepare(real=False)
                with torch.cuda.stream(S):
                    got, infos = _play(vs, fr, late_ms=PUSH_D_MS, marks=marks)
                S.synchronize()
            else:
                fr.prepare(real=True)
                e0 = torch.cuda.Event()
                St.sleep_ms(D)
                e0.record()
                t0 = time.perf_counter()
                with torch.cuda.stream(S):
                    got, infos = _play(vs, fr, marks=marks)
                S.synchronize()
                pending = not e0.query()
                wall = (time.perf_counter() - t0) * 1e3
                torch.cuda.synchronize()
            got = _host_frames(got)
            cuts = list(vs.cuts)
        finally:
            vs.close()
        same = [i for i, _ in got] == idx and St.same_bits(np.stack([f for _, f in got]), want)
        St.report(label, "probe " + probe, PUSH_D_MS if probe == "L" else D,
                  ("identical" if same else "DIFFERENT") + ("" if pending is None else ", e0 pending" if pending else ", e0 DONE"),
                  "D per push" if probe == "L" else "the sequence took %.1f ms; copy-stream placement %d of %d" % (wall, attempt + 1, placements))
        if same and pending is False and attempt + 1 < placements:
            St.keep_a_stream_alive()
            continue
        break
    assert [i for i, _ in warm] == idx and St.same_bits(np.stack([f for _, f in warm]), want), f"{label}: the undelayed session on S differs"
    assert (winfos, wcuts) == (rinfos, rcuts), (winfos, rinfos, wcuts, rcuts)
    assert same, f"{label}: probe {probe}: frames differ from the default-stream session's"
    assert (infos, cuts) == (rinfos, rcuts), (infos, rinfos, cuts, rcuts)
    if pending is not None:
        assert pending, f"{label}: the session ran on, or waited for, the null stream (on each of {placements} placements of its copy stream)"


def test_session_device_frames_on_a_side_stream():
    """E1: device frames, rgb24; every push's frame arrives late on S (the ring copy, the gather and the batch must all be behind it)."""
    frames = TS._frames_u8(10, SH, SW, seed=31)
    kw = dict(H=SH, W=SW, batch=SBATCH)
    ref = _session_reference("E1", _engine1, kw, frames, [True] * 10)
    assert ref[0] == list(range(10))
    eng = _engine1()
    try:
        _session_probe("session rgb24, device frames", "L", eng, kw, frames, [True] * 10, ref)
    finally:
        eng.close()


@pytest.mark.parametrize("probe", ["L", "N"])
def test_session_every_edge_kernel_on_a_side_stream(probe):
    """E2: NV12 in, P010 out at another raster, bt601: the input conversion, the 10-bit quantisation, the resampler and the 4:2:0 packing
    all run on the session's stream."""
    frames = TY._yuv_frames(9, SH, SW, "nv12", seed=32)
    kw = dict(H=SH, W=SW, batch=SBATCH, pixel_format="nv12", out_format="p010", matrix="bt601", out_size=(36, 54))
    ref = _session_reference("E2", _engine1, kw, frames, [True] * 9)
    assert ref[0] == list(range(9)) and ref[1].dtype == np.uint16 and ref[1].shape[1:] == (54, 54)
    eng = _engine1()
    try:
        _session_probe("session nv12 -> p010 36x54 bt601, device frames", probe, eng, kw, frames, [True] * 9, ref)
    finally:
        eng.close()


def test_session_mixed_pushes_with_scenes_on_a_side_stream():
    """E3: scene_cut=10 on content with two cuts, device (late) and host pushes alternating: the copy stream must fall in behind the
    decisions taken on the session's stream (scene_ev / decided_on_s).  Frames, cuts and every (scene_first, sad) equal the reference."""
    frames = TSC._scenes_u8((4, 3, 4), seed=33)
    sf = scene.scene_first(frames, threshold=10)
    assert list(sf) == [0] * 4 + [4] * 3 + [7] * 4
    mask = [k % 3 == 1 for k in range(11)]
    kw = dict(H=SH, W=SW, batch=SBATCH, scene_cut=10)
    ref = _session_reference("E3", _engine1, kw, frames, mask)
    assert ref[0] == list(range(11)) and ref[3] == [4, 7]
    assert ref[2] == [(int(a), s) for a, s in zip(sf, scene.frame_sads(frames))]
    eng = _engine1()
    try:
        _session_probe("session scene_cut=10, device / host pushes alternate", "L", eng, kw, frames, mask, ref)
    finally:
        eng.close()


def test_session_host_frames_complete_while_the_null_stream_sleeps():
    """E4: host frames in and out; the whole sequence, end() included, completes while the null stream spins."""
    frames = TS._frames_u8(10, SH, SW, seed=34)
    kw = dict(H=SH, W=SW, batch=SBATCH)
    ref = _session_reference("E4", _engine1, kw, frames, [False] * 10)
    eng = _engine1()
    try:
        _session_probe("session rgb24, host frames", "N", eng, kw, frames, [False] * 10, ref)
    finally:
        eng.close()


def test_session_scene_table_setup_while_the_null_stream_sleeps():
    """E5: the session is opened, pfnl_stream_scenes zeroes its table (a null-stream hipMemset) and the first two host frames are pushed
    (their sums run on the non-blocking copy stream) while the null stream spins.  The sads equal the reference; whether the setup call
    blocked until the spin ended is reported (either is allowed)."""
    St.require("N")
    frames = TSC._scenes_u8((4, 3, 4), seed=35)
    kw = dict(H=SH, W=SW, batch=SBATCH, scene_cut=10)
    ref = _session_reference("E5", _engine1, kw, frames, [False] * 11)
    S = St.side_stream()
    eng = _engine1()
    try:
        head, rest = Frames(frames[:2], [False] * 2), Frames(frames, [False] * 11)
        t0 = time.perf_counter()
        with torch.cuda.stream(S):
            with eng.open_stream(**kw) as vs:                                    # the warm-up: the same setup, undelayed
                _play(vs, head, stop=2)
        D = St.delay_ms((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
        e0 = torch.cuda.Event()
        St.sleep_ms(D)
        e0.record()
        with torch.cuda.stream(S):
            vs = eng.open_stream(**kw)
            got, infos = _play(vs, head, stop=2)
        pending = not e0.query()
        torch.cuda.synchronize()
        try:
            with torch.cuda.stream(S):
                rest.frames, rest.mask = rest.frames[2:], rest.mask[2:]
                more, minfos = _play(vs, rest)
            S.synchronize()
            got, infos = _host_frames(got + more), infos + minfos
        finally:
            vs.close()
        same = St.same_bits(np.stack([f for _, f in got]), ref[1]) and infos == ref[2]
        St.report("session setup (open, scenes, two host pushes)", "null asleep", D, "identical" if same else "DIFFERENT",
                  "setup returned while the null stream still span" if pending else "setup blocked until the spin ended")
        assert [i[1] for i in infos] == scene.frame_sads(frames), "the scene table's zeroing raced the sums on the copy stream"
        assert same and [i for i, _ in got] == ref[0]
    finally:
        eng.close()


def _range_weights():
    w = synth.synthetic_weights(GEOM1, seed=1)
    w["nlvsr/conv0/kernel"] = (w["nlvsr/conv0/kernel"] * 4e5).astype(np.float32)
    return w


def test_session_range_rerun_on_a_side_stream():
    """E6: the weights of test_session_recomputes_out_of_range_batches, device frames (late) on S: every frame equals the strict engine's
    (go_strict and the replay of check_batch run on S); the options are back after the last pop and after a close in mid-sequence."""
    St.require("L")
    lr_u8 = TS._frames_u8(7, 12, 20, seed=21)
    w = _range_weights()
    w["nlvsr/convmerge2/kernel"] = (w["nlvsr/convmerge2/kernel"] * 1e-6).astype(np.float32)
    strict = _engine1(w)
    strict.set_option("strict_fp32", "on")
    sr = strict.forward(np.ascontiguousarray(M.sliding_windows((lr_u8 / 255.).astype(np.float32), 7)))
    strict.close()
    assert np.isfinite(sr).all()
    want = M.quantise(sr[:, 0])
    S = St.side_stream()
    eng = _engine1(w)
    try:
        fr = Frames(lr_u8, [True] * 7)
        fr.prepare(real=False)
        with torch.cuda.stream(S):
            with eng.open_stream(12, 20, 3) as vs:
                got, _ = _play(vs, fr, late_ms=PUSH_D_MS)
                assert eng.get_option("strict_fp32") == "off" and eng.get_option("precision") == "fp32"     # the last pop has put them back
                S.synchronize()
                got = _host_frames(got)
        same = [i for i, _ in got] == list(range(7)) and St.same_bits(np.stack([f for _, f in got]), want)
        St.report("session range rerun, device frames", "probe L", PUSH_D_MS, "identical" if same else "DIFFERENT", "D per push; reference: the strict engine")
        assert same
        assert eng.range_flagged() is False
        fr.prepare(real=False)
        with torch.cuda.stream(S):
            with eng.open_stream(12, 20, 3) as vs:
                _play(vs, fr, late_ms=PUSH_D_MS, stop=7)                         # pushed, never ended
                vs.pop_ready()
                assert eng.get_option("strict_fp32") == "on"                    # the rest of the sequence runs strict
        assert eng.get_option("strict_fp32") == "off" and eng.get_option("precision") == "fp32" and eng.range_flagged() is False
    finally:
        eng.close()


def _with_forward(eng, vs, fr, x, late_ms, box):
    """the session's sequence with a plain device-pointer forward of x between pushes 7 and 8"""
    def forward():
        if late_ms is not None:
            St.sleep_ms(late_ms)
            St._as_int(box["xbuf"]).copy_(box["xpin"], non_blocking=True)
        box["y"] = eng.forward(box["xbuf"])
    return _play(vs, fr, late_ms=None if late_ms is None else PUSH_D_MS, at=(7, forward))


def test_plain_forward_between_pushes_on_the_sessions_stream():
    """E7: "Plain pfnl_forward calls on the handle remain possible between pushes: on the session's stream" - with a batch in flight the
    forward shares the handle's workspace with it, ordered by S alone.  Probe L on the forward's input and on every frame."""
    St.require("L")
    frames = TS._frames_u8(10, SH, SW, seed=36)
    x = synth.uniform_clips(1, 7, SH, SW, seed=37)
    orc = pfnl_fast.FastOracle(synth.synthetic_weights(GEOM1, seed=0), num_block=1).forward(x)

    def run(stream, probed):
        """the sequence on `stream` on a fresh engine; probed: once more behind the delays -> ([(frames, y)], the forward's D)"""
        eng = _engine1()
        fr = Frames(frames, [True] * 10)
        box = {"xbuf": St.to_device(x), "xpin": St.pinned_like(x)}
        outs, D = [], None
        try:
            with torch.cuda.stream(stream):
                with eng.open_stream(SH, SW, SBATCH) as vs:
                    for late in ([False, True] if probed else [False]):          # on S: the undelayed warm-up first
                        fr.prepare(real=not late)
                        if late:
                            St.fill_pattern(box["xbuf"])
                            torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        got, _ = _with_forward(eng, vs, fr, x, D if late else None, box)
                        stream.synchronize()
                        if not late:
                            D = St.delay_ms((time.perf_counter() - t0) * 1e3)    # (the whole sequence's wall time: no less than the forward's)
                        outs.append((_host_frames(got), box["y"].cpu().numpy()))
                        vs.reset()
        finally:
            eng.close()
        return outs, D

    ((ref_frames, ref_y),), _ = run(torch.cuda.default_stream(), False)
    err = float(np.abs(ref_y - orc).max())
    assert np.isfinite(ref_y).all() and err < TF.ABS_TOL, err
    ((warm_frames, warm_y), (got_frames, got_y)), D = run(St.side_stream(), True)
    same_y, same_f = St.same_bits(got_y, ref_y), St.same_bits(np.stack([f for _, f in got_frames]), np.stack([f for _, f in ref_frames]))
    St.report("forward between two pushes of a session", "probe L", D, f"forward {'identical' if same_y else 'DIFFERENT'}, frames {'identical' if same_f else 'DIFFERENT'}",
              "max err %.2g; frames: D per push %.0f ms" % (err, PUSH_D_MS))
    assert St.same_bits(warm_y, ref_y) and St.same_bits(np.stack([f for _, f in warm_frames]), np.stack([f for _, f in ref_frames]))
    assert same_y and same_f and [i for i, _ in got_frames] == list(range(10))


def test_session_reset_with_a_batch_in_flight_on_a_side_stream():
    """E8: reset() on S with a batch launched and never popped, then a second sequence (late frames): a fresh session's bytes."""
    St.require("L")
    a, b = TS._frames_u8(9, SH, SW, seed=38), TS._frames_u8(8, SH, SW, seed=39)
    kw = dict(H=SH, W=SW, batch=SBATCH)
    ref = _session_reference("E8", _engine1, kw, b, [True] * 8)
    S = St.side_stream()
    eng = _engine1()
    try:
        fa, fb = Frames(a, [True] * 9), Frames(b, [True] * 8)
        fb.prepare(real=False)
        with torch.cuda.stream(S):
            with eng.open_stream(**kw) as vs:
                _play(vs, fa, stop=9)                                           # the ninth push launches the second batch; nobody pops it
                assert vs.ready() > 0
                vs.reset()
                assert vs.ready() == 0
                got, _ = _play(vs, fb, late_ms=PUSH_D_MS)
                S.synchronize()
                got = _host_frames(got)
        same = [i for i, _ in got] == ref[0] and St.same_bits(np.stack([f for _, f in got]), ref[1])
        St.report("session reset with a batch in flight, second sequence", "probe L", PUSH_D_MS, "identical" if same else "DIFFERENT", "D per push")
        assert same
    finally:
        eng.close()


# ---- F. the asynchronous op hooks --------------------------------------------------------------------------------------------------------

def _hook_gather_windows():
    fr = np.random.default_rng(9).random((5, 4, 6, 3), dtype=np.float32)
    return [fr], lambda b: [ops.gather_windows(b[0], 1, 4, 7)], lambda r: np.array_equal(r[0], M.sliding_windows(fr, 7)[1:5]), ()


def _ring_case(T, with_scenes):
    F, cap, h, w, last, first, count = 40, 13, 16, 24, 30, 20, 4                # the interior, a wrapped ring; 16-byte reads
    seq = TS._frames_u8(F, h, w, 100 + T)
    sf = np.zeros((F,), np.int64)
    for f in range(1, F):
        sf[f] = f if f in (19, 22) else sf[f - 1]                               # "both sides" of test_gpu_scene's layouts
    lo, hi = max(0, first - T // 2), min(last, first + count - 1 + T // 2)
    ring, table = 255 - seq[:cap].copy(), np.full((cap,), 12345, np.int64)
    for f in range(lo, hi + 1):
        ring[f % cap], table[f % cap] = seq[f], sf[f]
    if with_scenes:
        want = (seq[scene.scene_windows_index(sf, T, last)[first:first + count]] / 255.).astype(np.float32)
        return [ring, table], lambda b: [ops.gather_windows_u8_scenes(b[0], b[1], last, first, count, T)], lambda r: St.same_bits(r[0], want), ()
    want = M.sliding_windows((seq[:last + 1] / 255.).astype(np.float32), T)[first:first + count]
    return [ring], lambda b: [ops.gather_windows_u8(b[0], last, first, count, T)], lambda r: St.same_bits(r[0], want), ()


def _hook_quantise_u8():
    sr = (np.random.default_rng(9).random((2, 1, 8, 12, 3), dtype=np.float32) * 1.4 - 0.2)
    sr.ravel()[:8] = [0.5 / 255, 1.5 / 255, 2.5 / 255, 254.5 / 255, 1.0, 0.0, -1.0, 2.0]
    return [sr], lambda b: [ops.quantise_u8(b[0])], lambda r: np.array_equal(r[0], M.quantise(sr)), ()


def _hook_quantise_u10():
    x = np.random.default_rng(1).uniform(-0.1, 1.1, 1 << 12).astype(np.float32)
    t = ((np.arange(1023) + 0.5) / 1023).astype(np.float32)                       # the ties of test_quantise_u10_equals_the_host_rule
    x = np.concatenate([x, np.nextafter(t, np.float32(-1)), t, np.nextafter(t, np.float32(2)), np.zeros(3, np.float32)])
    assert x.size % 4 == 0
    return [x], lambda b: [ops.quantise_u10(b[0])], lambda r: np.array_equal(r[0], depth10.quantise10(x)), ()


def _hook_yuv420_to_rgb():
    n, h, w = 3, 16, 64                                                         # 16-byte words
    frames = TY._yuv_frames(n, h, w, "nv12", seed=h * 1000 + w + n)
    out = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
    want = np.stack([yuv.to_rgb(f, "nv12", h, w, "bt601", False) for f in frames])
    return [frames], lambda b: [ops.yuv420_to_rgb(b[0], "nv12", h, w, "bt601", False, out=out)], lambda r: np.array_equal(r[0], want), (out,)


def _hook_rgb_to_yuv420():
    n, h, w = 3, 16, 64
    frames = TY._rgb_frames(n, h, w, seed=h * 1000 + w + 10 + n)
    out = torch.empty((n, h * 3 // 2, w), dtype=torch.uint8, device="cuda")
    want = np.stack([yuv.from_rgb(f, "i420", "bt709", True) for f in frames])
    return [frames], lambda b: [ops.rgb_to_yuv420(b[0], "i420", "bt709", True, out=out)], lambda r: np.array_equal(r[0], want), (out,)


def _hook_rgb_to_yuv420_u10():
    n, h, w = 3, 16, 24                                                         # 16-byte words (W % 8 == 0)
    frames = TD._rgb10_frames(n, h, w, seed=h * 1000 + w + n)
    out = torch.empty((n, h * 3 // 2, w), dtype=torch.uint16, device="cuda")
    want = np.stack([depth10.from_rgb10(f, "p010", "bt709", False) for f in frames])
    return [frames], lambda b: [ops.rgb_to_yuv420_u10(b[0], "p010", "bt709", False, out=out)], lambda r: np.array_equal(r[0], want), (out,)


def _hook_bicubic():
    x = np.random.default_rng(507).random((1, 5, 7, 3), dtype=np.float32)
    ref = pfnl_spec.resize_bicubic_tf1(x.astype(np.float64), 4)
    return [x], lambda b: [ops.bicubic(b[0], 4)], lambda r: r[0].shape == ref.shape and np.abs(r[0] - ref).max() < 2e-6, ()


def _hook_blur_decimate():
    hr = np.random.default_rng(15).random((1, 7, 7, 3), dtype=np.float32)
    ref = synth.blur_decimate(hr.astype(np.float64), 4)
    return [hr], lambda b: [ops.blur_decimate(b[0], 4)], lambda r: r[0].shape == ref.shape and np.abs(r[0] - ref).max() < 2e-6, ()


def _hook_score_y():
    truth, pred = TSY.content_pairs(11, 11, seed=11011)
    want = TSY.per_frame_metrics(truth, pred)

    def check(r):
        TSY.check_against_metrics(r[0], truth, pred, want, 4, "11x11 on the default stream")
        return True
    return [pred, truth], lambda b: [ops.score_y(b[0], b[1], 4)], check, ()


HOOKS = {"gather_windows": _hook_gather_windows, "gather_windows_u8": lambda: _ring_case(7, False), "gather_windows_u8_scenes": lambda: _ring_case(3, True),
         "quantise_u8": _hook_quantise_u8, "quantise_u10": _hook_quantise_u10, "yuv420_to_rgb": _hook_yuv420_to_rgb, "rgb_to_yuv420": _hook_rgb_to_yuv420,
         "rgb_to_yuv420_u10": _hook_rgb_to_yuv420_u10, "bicubic": _hook_bicubic, "blur_decimate": _hook_blur_decimate, "score_y": _hook_score_y}


def _default_stream_result(inputs, body, owned):
    dev = [St.to_device(a) for a in inputs]
    for t in owned:
        St.fill_pattern(t)
    torch.cuda.synchronize()
    res = body(dev)
    torch.cuda.synchronize()
    return [St.to_numpy(St._as_int(r).cpu(), r) for r in res]


@pytest.mark.parametrize("probe", ["L", "N"])
@pytest.mark.parametrize("hook", list(HOOKS))
def test_async_op_hook_on_a_side_stream(hook, probe):
    """The hooks documented as asynchronous on `stream`, at the smallest shape of their op tests that takes the wide-word form: the
    default-stream result holds the host rule of the op's own test; on S the bits are the same."""
    inputs, body, holds, owned = HOOKS[hook]()
    ref = _default_stream_result(inputs, body, owned)
    assert holds(ref), f"{hook}: the default-stream result misses the host rule"
    _verdict(St.Probe(f"op {hook}", St.side_stream(), inputs, body, owned=owned), probe, ref)


# ---- G. three hooks that synchronise before they return ---------------------------------------------------------------------------------

def _sync_chain():
    T, clips, H, W, split = TO._split_case("nfull0-ragged", TH._grid())
    rng = np.random.default_rng(len("nfull0-ragged") * 11 + T)
    x, res = (rng.normal(size=(clips * T, H, W, 64)).astype(np.float32) for _ in range(2))
    base = rng.normal(size=(clips, H, W, 64)).astype(np.float32)
    k2 = (rng.normal(size=(3, 3, 128, 64)) / 34.0).astype(np.float32)
    b = (rng.normal(size=64) * 0.1).astype(np.float32)
    sel = list(range(clips))

    def holds(r):
        ref = TO._chain_ref(x, base, res, k2, b, T, sel)
        return np.abs(TO._frames_of(r[0], T, sel) - ref).max() < TO.SPLIT16_OP_REL_TOL * max(1.0, np.abs(ref).max())
    return [x, base, res], lambda d: [ops.conv2_chain_ex(d[0], k2, b, d[1], d[2], T, split=split)], holds


def _sync_c1c10():
    T, clips, H, W, split = TO._split_case("nfull0-ragged", TH._grid())
    x, k1, b1, k10, b10 = TH._c1c10_data(T, clips, H, W)

    def holds(r):
        TH._c1c10_check(x, k1, b1, k10, b10, T, list(range(clips)), torch.from_numpy(r[0]), torch.from_numpy(r[1]))
        return True
    return [x], lambda d: list(ops.conv1_conv10_split16_ex(d[0], k1, b1, k10, b10, T, split=split)), holds


def _sync_nonlocal():
    B, T, H, W, sub = 1, 7, 4, 4, 2                                             # a single pooled key: the smallest of test_nonlocal_block_general
    rng = np.random.default_rng(T * 7 + H + 100 + sub)
    C = 12 * T
    x = rng.random((B, T, H, W, 3), dtype=np.float32)
    wg, ww = ((rng.normal(size=(1, 1, C, C)) * 0.1).astype(np.float32) for _ in range(2))
    bg, bw = ((rng.normal(size=C) * 0.05).astype(np.float32) for _ in range(2))

    def holds(r):
        f = lambda a: a.astype(np.float64)                                       # noqa: E731
        stack = np.concatenate([x[:, t] for t in range(T)], -1).astype(np.float64)
        z = pfnl_spec.nonlocal_block(pfnl_spec.space_to_depth2(stack), f(wg), f(bg), f(ww), f(bw), nltype=1, sub_sample=sub)
        return np.abs(r[0] - (stack + pfnl_spec.depth_to_space2(z))).max() < 2e-5
    return [x], lambda d: [ops.nonlocal_block(d[0], wg, bg, ww, bw, nltype=1, sub_sample=sub)], holds


SYNC_HOOKS = {"conv2_chain_ex split": _sync_chain, "conv1_conv10_split16_ex split": _sync_c1c10, "nonlocal_block sub_sample=2": _sync_nonlocal}


@pytest.mark.parametrize("hook", list(SYNC_HOOKS))
def test_synchronising_op_hook_on_a_side_stream(hook):
    """Hooks that upload a weight pack with a pageable hipMemcpy and synchronise before they return (Probe L only: the upload goes through
    the null stream): the cut launch and its finalize kernel, and the pooled non-local block, run behind the late input on S."""
    inputs, body, holds = SYNC_HOOKS[hook]()
    ref = _default_stream_result(inputs, body, ())
    assert holds(ref), f"{hook}: the default-stream result misses the bound of the op's own test"
    _verdict(St.Probe(f"op {hook}", St.side_stream(), inputs, body), "L", ref)


# ---- H. the range flag of an asynchronous call ---------------------------------------------------------------------------------------------

def test_range_flag_of_an_asynchronous_forward_on_a_side_stream():
    """conv0 x 4e5: forward_device on S is flagged; read after the caller's own synchronise the flag is set once, then clear; an in-range
    forward on S leaves it clear."""
    St.require("L")
    S = St.side_stream()
    x = synth.uniform_clips(1, 7, 16, 24, seed=3)
    eng = _engine1(_range_weights())
    try:
        xd = torch.from_numpy(x).cuda()
        out = torch.empty(eng.out_shape(1, 16, 24), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        with torch.cuda.stream(S):
            eng.forward_device(xd.data_ptr(), out.data_ptr(), 1, 16, 24, stream=S.cuda_stream)     # (the warm-up)
        S.synchronize()
        eng.range_flagged()
        with torch.cuda.stream(S):
            eng.forward_device(xd.data_ptr(), out.data_ptr(), 1, 16, 24, stream=S.cuda_stream)
        S.synchronize()
        first, second = eng.range_flagged(), eng.range_flagged()
        finite = bool(torch.isfinite(out).all())
        eng.load_weights(synth.synthetic_weights(GEOM1, seed=1))
        with torch.cuda.stream(S):
            eng.forward_device(xd.data_ptr(), out.data_ptr(), 1, 16, 24, stream=S.cuda_stream)
        S.synchronize()
        third = eng.range_flagged()
        St.report("range flag of forward_device", "flag", None, f"after the caller's synchronise {first}, then {second}; in-range forward {third}")
        assert first is True and second is False and not finite
        assert third is False and bool(torch.isfinite(out).all())
    finally:
        eng.close()
