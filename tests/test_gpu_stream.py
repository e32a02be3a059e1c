"""The streaming session on a real MI355X (include/pfnl_hip.h pfnl_stream_*, pfnl_amd/stream.py): uint8 frames pushed one at a time
give the bytes of the explicit path - gather_windows, forward, quantise_u8 on the same batches - and of the harness; the ring gather
dequantises bit for bit as the harness does; the bounds, reset and the range fence behave as documented."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from conftest import load_golden  # noqa: E402
from pfnl_amd import model as M  # noqa: E402
from pfnl_amd import ops, synth  # noqa: E402
from pfnl_amd.engine import PFNLEngine  # noqa: E402
from pfnl_amd.spec import PFNLGeometry  # noqa: E402


def _engine_with(geom, w, precision="fp32"):
    e = PFNLEngine(geom, device=0)
    e.load_weights(w)
    if precision != "fp32":
        e.set_option("precision", precision)
    return e


def _frames_u8(F, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(F, H, W, 3), dtype=np.uint8)


def _stream_all(vs, frames, device=False):
    """push one frame at a time, pop after every push, then end: [(index, frame)] in delivery order"""
    got = []
    for f in frames:
        got += vs.push(torch.from_numpy(f).cuda() if device else f)
        got += vs.pop_ready()
    got += vs.end()
    return got


def _explicit(eng, frames_u8, batch, T):
    """the same batches through the single ops on `eng`: [F,sH,sW,3] uint8"""
    F = frames_u8.shape[0]
    dev = torch.from_numpy((frames_u8 / 255.).astype(np.float32)).cuda()
    outs = []
    for first in range(0, F, batch):
        count = min(batch, F - first)
        outs.append(ops.quantise_u8(eng.forward(ops.gather_windows(dev, first, count, T)))[:, 0].cpu().numpy())
    return np.concatenate(outs)


# ---- 1. the op --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [3, 5, 7])
@pytest.mark.parametrize("H,W", [(6, 10), (16, 24)])        # H*W*3 = 180 (4-byte reads) and 1152 (16-byte reads)
def test_gather_windows_u8_equals_the_harness_expression(T, H, W):
    F, cap = 40, 13
    seq = _frames_u8(F, H, W, 100 + T)
    seq.reshape(F, -1)[::2, :180] = np.arange(180, dtype=np.uint8)[None, :]
    seq.reshape(F, -1)[1::2, :180] = np.arange(76, 256, dtype=np.uint8)[None, :]
    assert len(np.unique(seq[:2])) == 256                                           # all 256 byte values, in two neighbouring frames
    cases = [(0, 0, 1),                    # a sequence of one frame: every slot clamps to it
             (9, 0, 4),                    # the clamp at frame 0
             (39, 36, 4),                  # the clamp at `last`; first > cap: a wrapped ring
             (30, 20, 5),                  # the interior, wrapped
             (2, 1, 2)]                    # both clamps in one window (T = 7)
    for last, first, count in cases:
        lo, hi = max(0, first - T // 2), min(last, first + count - 1 + T // 2)
        assert hi - lo + 1 <= cap
        ring = 255 - seq[:cap].copy()                                               # slots the windows do not name hold other bytes
        for f in range(lo, hi + 1):
            ring[f % cap] = seq[f]
        got = ops.gather_windows_u8(torch.from_numpy(ring).cuda(), last, first, count, T).cpu().numpy()
        want = M.sliding_windows((seq[:last + 1] / 255.).astype(np.float32), T)[first:first + count]
        assert got.dtype == np.float32 and got.shape == want.shape == (count, T, H, W, 3)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (T, H, W, last, first, count)   # bit for bit


# ---- 2. the session equals the explicit path ------------------------------------------------------------------------------------------
CASES = [(1, 1, 16, 24, 1), (3, 1, 16, 24, 1), (5, 3, 16, 24, 1), (7, 3, 16, 24, 1), (9, 4, 16, 24, 1), (12, 4, 16, 24, 1), (2, 5, 16, 24, 1),
         (6, 2, 64, 64, 2)]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("F,batch,H,W,nb", CASES)
def test_session_equals_explicit_path_byte_for_byte(F, batch, H, W, nb, precision):
    geom = PFNLGeometry(num_block=nb)
    w = synth.synthetic_weights(geom, seed=0)
    eng, eng2 = _engine_with(geom, w, precision), _engine_with(geom, w, precision)
    frames = _frames_u8(F, H, W, seed=F * 10 + batch)
    with eng.open_stream(H, W, batch) as vs:
        got = _stream_all(vs, frames)
    assert [i for i, _ in got] == list(range(F))
    want = _explicit(eng2, frames, batch, geom.num_frames)
    sr = np.stack([f for _, f in got])
    assert sr.dtype == np.uint8 and sr.shape == want.shape == (F, 4 * H, 4 * W, 3)
    assert np.array_equal(sr, want)
    assert eng.get_option("precision") == precision and eng.get_option("strict_fp32") == "off"
    eng.close()
    eng2.close()


# ---- 3. / 4. the golden sequence and the harness ------------------------------------------------------------------------------------------
def _golden_model(tmp_path):
    from model.pfnl import PFNL
    m = PFNL()
    m.num_block = 1
    m.save_dir = str(tmp_path / "none")
    m.set_weights(synth.synthetic_weights(PFNLGeometry(num_block=1), seed=0))
    return m


def test_session_reproduces_the_golden_harness_frames(tmp_path):
    gd = load_golden("harness_5x16x24_nb1")
    with _golden_model(tmp_path).open_stream(16, 24, batch=3) as vs:
        got = _stream_all(vs, gd["lr_u8"])
    assert [i for i, _ in got] == list(range(5))
    diff = np.abs(np.stack([f for _, f in got]).astype(np.int32) - gd["sr_u8"].astype(np.int32))
    print("max |diff| %d, share of differing bytes %.3g" % (diff.max(), (diff > 0).mean()))
    assert diff.max() <= 1 and (diff > 0).mean() < 1e-3           # rounding ties only: test_dropin_class_and_harness's bound


def test_session_gives_the_bytes_of_test_video_lr(tmp_path):
    from PIL import Image
    gd = load_golden("harness_5x16x24_nb1")
    seq = tmp_path / "seq0"
    (seq / "blur4").mkdir(parents=True)
    for i, im in enumerate(gd["lr_u8"]):
        Image.fromarray(im).save(seq / "blur4" / f"{i:04d}.png")
    m = _golden_model(tmp_path)
    m.test_video_lr(str(seq), name="result", part=2)              # 5 frames, part=2 -> num_once=3
    pngs = np.stack([np.asarray(Image.open(p)) for p in sorted((seq / "result").glob("*.png"))])
    with m.open_stream(16, 24, batch=3) as vs:
        got = _stream_all(vs, gd["lr_u8"])
    assert np.array_equal(np.stack([f for _, f in got]), pngs)


# ---- 5. device pointers ---------------------------------------------------------------------------------------------------------------
def test_device_frames_give_the_same_bytes():
    geom = PFNLGeometry(num_block=1)
    eng = _engine_with(geom, synth.synthetic_weights(geom, seed=0))
    frames = _frames_u8(8, 16, 24, seed=5)
    with eng.open_stream(16, 24, 3) as vs:
        host = _stream_all(vs, frames)
        vs.reset()
        dev = _stream_all(vs, frames, device=True)
    assert all(isinstance(f, np.ndarray) for _, f in host)
    assert all(torch.is_tensor(f) and f.is_cuda and f.dtype == torch.uint8 for _, f in dev)
    assert [i for i, _ in dev] == [i for i, _ in host] == list(range(8))
    assert np.array_equal(np.stack([f.cpu().numpy() for _, f in dev]), np.stack([f for _, f in host]))
    eng.close()


# ---- 6. readiness and the bound ---------------------------------------------------------------------------------------------------------
def test_readiness_and_the_undelivered_bound():
    geom = PFNLGeometry(num_block=1)
    T = geom.num_frames
    eng = _engine_with(geom, synth.synthetic_weights(geom, seed=0))
    frames = _frames_u8(12, 16, 24, seed=6)
    want = _explicit(eng, frames[:9], 1, T)
    lib = eng._lib
    raw_push = lambda vs, f: lib.pfnl_stream_push(vs._s, f.ctypes.data_as(C.c_void_p), 0)   # noqa: E731
    with eng.open_stream(16, 24, 1) as vs:
        for k in range(T // 2):
            assert raw_push(vs, frames[k]) == 0 and vs.ready() == 0 and vs.pop() is None     # got = 0 is not an error
        for k in range(T // 2, T // 2 + 3):                                                   # then one per push
            assert raw_push(vs, frames[k]) == 0 and vs.ready() == 1
            i, f = vs.pop()
            assert i == k - T // 2 and np.array_equal(f, want[i]) and vs.ready() == 0
        k = T // 2 + 3
        assert raw_push(vs, frames[k]) == 0 and vs.ready() == 1
        assert raw_push(vs, frames[k + 1]) == 0 and vs.ready() == 2                           # 2 * batch undelivered frames
        assert raw_push(vs, frames[k + 2]) == -2 and b"pop first" in lib.pfnl_last_error()    # PFNL_ERR_STATE, nothing changed
        assert vs.ready() == 2
        i, f = vs.pop()
        assert i == 3 and np.array_equal(f, want[3])
        assert raw_push(vs, frames[k + 2]) == 0 and vs.ready() == 2                           # the refused frame, now accepted
        # pushed: T/2 + 6 = 9 frames, delivered 4, launched 6: after the end the T/2 frames behind them are ready as well
        assert lib.pfnl_stream_end(vs._s) == 0 and vs.ready() == 5
        assert raw_push(vs, frames[0]) == -2 and b"pfnl_stream_end" in lib.pfnl_last_error()  # push after end
        rest = vs.pop_ready()
        assert [i for i, _ in rest] == [4, 5, 6, 7, 8] and vs.ready() == 0 and vs.pop() is None
        assert np.array_equal(np.stack([f for _, f in rest]), want[4:])
        s2 = C.c_void_p()                                                                     # one open session per handle
        assert lib.pfnl_stream_open(eng._h, 16, 24, 1, None, C.byref(s2)) == -2
    with eng.open_stream(16, 24, 2) as vs:                                                    # ... and after close the next one opens
        y = eng.forward(synth.uniform_clips(1, T, 16, 24, seed=1))                            # plain forwards stay possible
        assert np.isfinite(y).all()
        assert vs.end() == []                                                                 # F = 0: nothing launches
    eng.close()


# ---- 7. reset ---------------------------------------------------------------------------------------------------------------------------
def test_reset_starts_a_fresh_sequence_and_options_survive():
    geom = PFNLGeometry(num_block=1)
    w = synth.synthetic_weights(geom, seed=0)
    eng = _engine_with(geom, w)
    eng.set_option("split16_mid", "off")
    eng.set_option("nonlocal", "f32")
    before = {k: eng.get_option(k) for k in eng.OPTION_KEYS}
    a, b = _frames_u8(9, 16, 24, seed=7), _frames_u8(5, 16, 24, seed=8)
    with eng.open_stream(16, 24, 2) as vs:
        for f in a[:7]:
            vs.push(f)                                              # two batches of A launched, the second never popped
        assert vs.ready() > 0
        vs.reset()
        assert vs.ready() == 0
        second = _stream_all(vs, b)
    with eng.open_stream(16, 24, 2) as vs:
        fresh = _stream_all(vs, b)
    assert [i for i, _ in second] == [i for i, _ in fresh] == list(range(5))
    assert np.array_equal(np.stack([f for _, f in second]), np.stack([f for _, f in fresh]))
    assert {k: eng.get_option(k) for k in eng.OPTION_KEYS} == before
    eng.close()


# ---- 8. the range fence -------------------------------------------------------------------------------------------------------------------
def test_session_recomputes_out_of_range_batches():
    """The weights of test_harness_reruns_out_of_range_batches: conv0 x 4e5 takes the activations beyond binary16's range (a numeric
    overflow of the f16-pipe kernels' operands, flagged by the tail kernel), convmerge2 x 1e-6 brings the result back onto the byte
    scale.  7 frames in batches of 3, 3, 1: every frame equals the strict engine's."""
    lr_u8 = _frames_u8(7, 12, 20, seed=21)
    geom = PFNLGeometry(num_block=1)
    w = synth.synthetic_weights(geom, seed=1)
    w["nlvsr/conv0/kernel"] = (w["nlvsr/conv0/kernel"] * 4e5).astype(np.float32)
    w["nlvsr/convmerge2/kernel"] = (w["nlvsr/convmerge2/kernel"] * 1e-6).astype(np.float32)
    eng = _engine_with(geom, w)
    was = eng.get_option("strict_fp32")
    with eng.open_stream(12, 20, 3) as vs:
        got = _stream_all(vs, lr_u8)
        assert eng.get_option("strict_fp32") == was                 # end + the last pop have put it back already
    strict = _engine_with(geom, w)
    strict.set_option("strict_fp32", "on")
    lrs = (lr_u8 / 255.).astype(np.float32)
    sr = strict.forward(np.ascontiguousarray(M.sliding_windows(lrs, 7)))
    assert np.isfinite(sr).all()
    assert [i for i, _ in got] == list(range(7))
    assert np.array_equal(np.stack([f for _, f in got]), M.quantise(sr[:, 0]))
    assert eng.get_option("strict_fp32") == was == "off" and eng.range_flagged() is False
    y = eng.forward(np.ascontiguousarray(M.sliding_windows(lrs, 7)[:1]))   # back on its default kernels: the host-pointer call reruns by itself
    assert np.isfinite(y).all() and eng.range_reruns() == 1
    # a session that is closed in the middle of such a sequence restores the option as well
    with eng.open_stream(12, 20, 3) as vs:
        for f in lr_u8:
            vs.push(f)
            vs.pop_ready()
        assert eng.get_option("strict_fp32") == "on"                # the rest of the sequence runs strict
    assert eng.get_option("strict_fp32") == "off"
    eng.close()
    strict.close()


def test_session_recomputes_out_of_range_batches_bf16():
    """precision=bf16: strict_fp32 changes no kernel there (its non-local block and conv0 keep binary16 operands), so the recomputation -
    and the rest of the sequence - runs at precision=fp32, strict_fp32=on, and the engine is back at bf16 afterwards, as in
    test_harness_reruns_out_of_range_batches_bf16.  That test leaves the range through float frames x 600; uint8 frames are in [0, 1]
    whatever their bytes, so here the non-local block itself leaves it: g's bias 200 through w = 600 I is a constant 1.2e5 on the
    block's output (x + NL(x), fp32), which conv0 of this precision takes as a binary16 operand: inf."""
    lr_u8 = _frames_u8(7, 12, 20, seed=22)
    geom = PFNLGeometry(num_block=1)
    Cn = 12 * geom.num_frames
    w = synth.synthetic_weights(geom, seed=1)
    w["nlvsr/nlblock_0/g/g/bias"] = np.full((Cn,), 200.0, np.float32)
    w["nlvsr/nlblock_0/w/w/kernel"] = (600.0 * np.eye(Cn, dtype=np.float32)).reshape(1, 1, Cn, Cn)
    w["nlvsr/conv0/kernel"] = (w["nlvsr/conv0/kernel"] * 1e-3).astype(np.float32)   # conv0 of 1.2e5-scale inputs back to O(1) activations
    eng = _engine_with(geom, w, "bf16")
    lrs = (lr_u8 / 255.).astype(np.float32)
    with pytest.raises(RuntimeError):                               # a bf16 forward of these frames reports the range (host-pointer call)
        eng.forward(np.ascontiguousarray(M.sliding_windows(lrs, 7)[:1]))
    with eng.open_stream(12, 20, 3) as vs:
        got = _stream_all(vs, lr_u8)
        assert eng.get_option("precision") == "bf16" and eng.get_option("strict_fp32") == "off"
    strict = _engine_with(geom, w)
    strict.set_option("strict_fp32", "on")
    sr = strict.forward(np.ascontiguousarray(M.sliding_windows(lrs, 7)))
    assert np.isfinite(sr).all()
    assert [i for i, _ in got] == list(range(7))
    assert np.array_equal(np.stack([f for _, f in got]), M.quantise(sr[:, 0]))   # every batch: the first one raised the flag
    assert eng.range_flagged() is False
    assert eng.get_option("precision") == "bf16" and eng.get_option("strict_fp32") == "off"   # the caller's configuration is back
    eng.close()
    strict.close()
