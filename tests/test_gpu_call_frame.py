"""What a call of pfnl_forward, pfnl_forward_ensemble and pfnl_forward_tiled does around its body (the call frame), on a
real MI355X: mixed pointer kinds, the rerun behind a graph replay, the precision=bf16 refusal and the order in which each entry reports a
misuse.  The three entries are driven through PFNLEngine._forward and the library itself, so that every pointer kind can meet every entry;
the all-host call of the same entry on the same engine is the reference, byte for byte."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from pfnl_amd import _capi, synth  # noqa: E402
from pfnl_amd.engine import PFNLEngine, tile_argument  # noqa: E402
from pfnl_amd.spec import PFNLGeometry  # noqa: E402

GEOM = PFNLGeometry(num_block=1)
H, W = 16, 24
TILE = (16, 16, 4, 1)                 # 16 x 24 under it: one row of two tiles (origins 0 and 8), a run each - the general tiled path
ENTRIES = {"plain": (1, None), "ensemble": (2, None), "tiled": (1, TILE)}       # entry -> (members, tiling)

MSG_BF16 = ("a precision=bf16 forward produced non-finite values: the input was not finite, or it left the range of the binary16 operands of "
            "this precision's non-local block and conv0 (inputs on a [0,1] scale, |x| < ~350). precision=fp32 covers the whole fp32 range")
MSG_FP32 = ("a device-pointer forward since the last check produced non-finite values: an operand left the range of the f16-pipe kernels "
            "(|x| < 65504; the non-local block: inputs on a [0,1] scale) or the input was not finite. Re-run with "
            "pfnl_set_option(h, \"strict_fp32\", \"on\") (f32-MFMA kernels: the reference's range), or use host pointers")


def _weights(overflow):
    """synth weights; overflow: conv0 x 4e5 as in test_split16_domain_activation_overflow_is_caught - the trunk leaves binary16's range"""
    w = dict(synth.synthetic_weights(GEOM, seed=1))
    if overflow:
        w["nlvsr/conv0/kernel"] = (w["nlvsr/conv0/kernel"] * 4e5).astype(np.float32)
    return w


def _engine(overflow=False):
    e = PFNLEngine(GEOM, device=0)
    e.load_weights(_weights(overflow))
    return e


def _ptr(a):
    return C.c_void_p(a.data_ptr()) if torch.is_tensor(a) else a.ctypes.data_as(C.c_void_p)


def _call(eng, entry, x, in_dev, out_dev):
    """one call of `entry` with the given pointer kinds on stream NULL; the status and the output container (NaN before the call)"""
    n, tile = ENTRIES[entry]
    B = x.shape[0]
    xin = torch.from_numpy(x).cuda() if in_dev else x
    shape = eng.out_shape(B, H, W)
    out = torch.full(shape, float("nan"), dtype=torch.float32, device="cuda") if out_dev else np.full(shape, np.nan, np.float32)
    torch.cuda.synchronize()                                                     # the operands are in place before the call starts
    status = eng._forward(n, _ptr(xin), int(in_dev), _ptr(out), int(out_dev), B, H, W, None, tile_argument(tile, x.shape))
    return status, out


def _read_on_another_stream(t):
    """the bytes of device tensor `t` as a non-blocking stream of its own sees them now: nothing here waits for any other stream"""
    side = torch.cuda.Stream()
    host = torch.empty(t.shape, dtype=t.dtype).pin_memory()
    with torch.cuda.stream(side):
        host.copy_(t, non_blocking=True)
    side.synchronize()
    return host.numpy().copy()


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- mixed pointer kinds ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overflow", [False, True], ids=["in_range", "overflow"])
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_mixed_pointer_kinds_are_synchronous_calls(entry, overflow):
    """host in / device out and device in / host out: the all-host call's bytes, complete when the call returns (the device `out` is read
    from another stream, the call's own stream never synchronised here); with the overflow weights each such call reads its flag (slot 0),
    reruns once and returns finite values, and leaves nothing in slot 1 for pfnl_sync."""
    eng = _engine(overflow)
    x = synth.uniform_clips(2, 7, H, W, seed=3)
    per_call = 1 if overflow else 0
    status, want = _call(eng, entry, x, False, False)
    assert status == 0 and np.isfinite(want).all() and eng.range_reruns() == per_call
    for k, (in_dev, out_dev) in enumerate([(False, True), (True, False)]):
        status, out = _call(eng, entry, x, in_dev, out_dev)
        got = _read_on_another_stream(out) if out_dev else out
        assert status == 0, (entry, in_dev, out_dev, eng._lib.pfnl_last_error())
        assert np.isfinite(got).all(), (entry, in_dev, out_dev)
        assert _same(got, want), (entry, in_dev, out_dev, float(np.abs(got - want).max()))
        assert eng.range_reruns() == (k + 2) * per_call, (entry, in_dev, out_dev)
    eng.sync()                                                                   # slot 1 is untouched: nothing to report
    assert eng.range_flagged() is False
    eng.close()


# ---- the rerun behind a graph replay ---------------------------------------------------------------------------------------------------
def test_a_flagged_graph_replay_reruns_once_per_call():
    """graph=on with the overflow weights, four host-pointer calls at one shape - eager, capture + replay, replay, replay: each counts one
    rerun, returns finite values and equals the graph=off result; a device-pointer replay stays asynchronous: non-finite, and pfnl_sync
    reports the range error once."""
    eng = _engine(overflow=True)
    x = synth.uniform_clips(1, 7, H, W, seed=3)
    eng.set_option("graph", "off")
    y_off = eng.forward(x)
    assert eng.range_reruns() == 1 and np.isfinite(y_off).all()
    eng.set_option("graph", "on")
    for k in range(4):
        y = eng.forward(x)
        assert eng.range_reruns() == 2 + k, k
        assert np.isfinite(y).all(), k
        assert _same(y, y_off), (k, float(np.abs(y - y_off).max()))
    eng.sync()                                                                   # the synchronous calls left slot 1 alone
    xd = torch.from_numpy(x).cuda()
    for k in range(3):                                                           # slot 1 has a graph of its own: eager, capture + replay, replay
        yd = eng.forward(xd)
    torch.cuda.synchronize()
    assert not torch.isfinite(yd).all()
    assert eng.range_reruns() == 5
    with pytest.raises(_capi.PFNLHipError) as ei:
        eng.sync()
    assert str(ei.value) == "libpfnl_hip status -7: " + MSG_FP32
    eng.sync()                                                                   # once: the flag was taken
    eng.close()


# ---- the precision=bf16 refusal --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_bf16_refuses_a_flagged_host_pointer_call(entry):
    """precision=bf16 has no f32-MFMA rerun: a host-pointer call whose flag is set returns PFNL_ERR_RANGE with the bf16 text, counts no
    rerun, and the handle serves the next call.  The plain entry runs under graph=on, so its second and third call are replays."""
    eng = _engine()
    eng.set_option("precision", "bf16")
    if entry == "plain":
        eng.set_option("graph", "on")
    x = synth.uniform_clips(1, 7, H, W, seed=3)
    bad = x.copy()
    bad[0, 3, 5, 12, 1] = np.inf                                                 # column 12: in both tiles of the tiled entry
    for k in range(3):
        status, _ = _call(eng, entry, bad, False, False)
        assert status == -7, (entry, k, status)
        assert eng._lib.pfnl_last_error().decode() == MSG_BF16, (entry, k)
        assert eng.range_reruns() == 0
    status, y = _call(eng, entry, x, False, False)
    assert status == 0 and np.isfinite(y).all() and eng.range_reruns() == 0
    eng.sync()
    eng.close()


# ---- what each entry refuses, and in which order ---------------------------------------------------------------------------------------
M_NULL = "NULL argument"
M_STATE = "pfnl_finalize_weights has not been called"
M_POS = "B, H, W must be positive"
M_EVEN = "H and W must be even (space_to_depth(2), reference model/pfnl.py:57)"
M_N = "ensemble: n must be 1, 2, 4 or 8"
M_TILE = "tile: 2 * pad must be smaller than the tile extent where the axis is split"
GOOD_TILE, BAD_TILE = TILE, (8, 8, 4, 1)     # tile_geom.h bounds a tile's size by its margin only: 2 * pad < extent on a split axis

# (entry, finalised, B, H, n, tiling) -> (status, message); -1 PFNL_ERR_INVALID, -2 PFNL_ERR_STATE
REFUSALS = [
    ("plain", True, 1, 17, 1, None, -1, M_EVEN),
    ("plain", True, 0, 16, 1, None, -1, M_POS),
    ("plain", False, 1, 16, 1, None, -2, M_STATE),
    ("plain", False, 0, 16, 1, None, -2, M_STATE),                               # the unfinalised handle is reported second, before the shape
    ("ensemble", True, 1, 17, 2, None, -1, M_EVEN),
    ("ensemble", True, 0, 16, 2, None, -1, M_POS),
    ("ensemble", True, 1, 16, 3, None, -1, M_N),
    ("ensemble", False, 1, 16, 2, None, -2, M_STATE),
    ("ensemble", False, 0, 16, 2, None, -2, M_STATE),
    ("ensemble", False, 1, 16, 3, None, -1, M_N),                                # n comes first of all
    ("tiled", True, 1, 17, 1, GOOD_TILE, -1, M_EVEN),
    ("tiled", True, 0, 16, 1, GOOD_TILE, -1, M_POS),
    ("tiled", True, 1, 16, 3, GOOD_TILE, -1, M_N),
    ("tiled", True, 1, 16, 1, BAD_TILE, -1, M_TILE),
    ("tiled", False, 1, 16, 1, GOOD_TILE, -2, M_STATE),
    ("tiled", False, 1, 16, 1, BAD_TILE, -1, M_TILE),                            # a refused tiling is reported before the unfinalised handle
    ("tiled", False, 0, 16, 1, GOOD_TILE, -1, M_POS),                            # ... and so is the shape
    ("tiled", False, 1, 16, 1, None, -2, M_STATE),                               # NULL tiling: the ensemble entry's (n == 1: the plain entry's) order
    ("tiled", False, 0, 16, 2, None, -2, M_STATE),
]


def test_refusals_per_entry():
    lib = _capi.load_library()
    ready, bare = _engine(), PFNLEngine(GEOM, device=0)                          # bare: weights never loaded
    x = np.zeros((1, 7, 18, W, 3), np.float32)                                   # room for every shape below; no refused call reads it
    y = np.zeros(ready.out_shape(1, 18, W), np.float32)
    for entry, finalised, B, Hc, n, tile, status, msg in REFUSALS:
        h = (ready if finalised else bare)._h
        a = (h, _ptr(x), 0, _ptr(y), 0, B, Hc, W)
        if entry == "plain":
            got = lib.pfnl_forward(*a, None)
        elif entry == "ensemble":
            got = lib.pfnl_forward_ensemble(*a, n, None)
        else:
            got = lib.pfnl_forward_tiled(*a, None if tile is None else C.byref(_capi.pfnl_tiling(*tile)), n, None)
        case = (entry, finalised, B, Hc, n, tile)
        assert got == status, (case, got, lib.pfnl_last_error())
        assert lib.pfnl_last_error().decode() == msg, case
    for entry in ENTRIES:                                                        # a NULL pointer: first for the plain entry, behind n (and the
        n, tile = ENTRIES[entry]                                                 # forwarding rules) for the other two
        a = (ready._h, None, 0, _ptr(y), 0, 1, H, W)
        got = {"plain": lambda: lib.pfnl_forward(*a, None), "ensemble": lambda: lib.pfnl_forward_ensemble(*a, n, None),
               "tiled": lambda: lib.pfnl_forward_tiled(*a, C.byref(_capi.pfnl_tiling(*tile)), n, None)}[entry]()
        assert got == -1 and lib.pfnl_last_error().decode() == M_NULL, entry
    assert ready.range_reruns() == 0
    ready.sync()
    ready.close()
    bare.close()
