"""The streaming session's settings in all pairs and across resets, on a real MI355X (include/pfnl_hip.h pfnl_stream_*;
pfnl_amd/csrc/capi_stream.hip candidate_refused, apply_setting; pfnl_amd/csrc/stream_route.h): tests/session_model.py states the session on
the host, and here the library delivers the model's bytes -

A. freshly opened, for every row of the pairwise array;
B. as ONE open session taken from row to row through the setters, pfnl_stream_reset between the sequences, in the array's order and in its
   reverse, every fourth step with the previous sequence abandoned while its batches are in flight, and back at the defaults at the end;
C. after a setter call the setting must refuse, which leaves no trace.

Byte for byte, no tolerance anywhere.  The array has 481 rows for 3288 legal pairs of values (481 of them input side x output side, the
lower bound).  Batch and weights have no setter, so a walk is one open session per (weights, batch) over the rows that have them.
On the MI355X the module's 119 cases take 27 s of wall time, beside 431 s for the rest of the ``-m gpu`` suite (1992 tests)."""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import session_model as M  # noqa: E402
from pfnl_amd import _capi, synth  # noqa: E402
from pfnl_amd import model as PM  # noqa: E402
from pfnl_amd.engine import PFNLEngine  # noqa: E402
from pfnl_amd.spec import PFNLGeometry  # noqa: E402

ROWS = M.covering_rows()
FRESH = M.chunks(ROWS)


def _walks():
    """(order, key, the row ahead of the chunk or None, the chunk's rows, the walk's step of its first row)"""
    out = []
    for order, rows in (("array", ROWS), ("reverse", ROWS[::-1])):
        for key, sub in M.walk_keys(rows).items():
            parts = M.chunks(sub)
            for k, part in enumerate(parts):
                out.append((order, key, parts[k - 1][-1] if k else None, part, 16 * k))
    return out


WALKS = _walks()


def _weights(geom, fence):
    """ordinary weights, or those of tests/test_gpu_stream.py test_session_recomputes_out_of_range_batches: conv0 x 4e5 takes the activations
    beyond binary16's range, convmerge2 x 1e-6 brings the result back onto the byte scale"""
    if not fence:
        return synth.synthetic_weights(geom, seed=0)
    w = synth.synthetic_weights(geom, seed=1)
    w["nlvsr/conv0/kernel"] = (w["nlvsr/conv0/kernel"] * 4e5).astype(np.float32)
    w["nlvsr/convmerge2/kernel"] = (w["nlvsr/convmerge2/kernel"] * 1e-6).astype(np.float32)
    return w


@pytest.fixture(scope="module")
def engines():
    """fence -> (the engine under test, the engine of the plain session): one PF block, the same weights"""
    geom = PFNLGeometry(num_block=1)
    made = {}
    for fence in (False, True):
        w = _weights(geom, fence)
        made[fence] = []
        for _ in range(2):
            e = PFNLEngine(geom, device=0)
            e.load_weights(w)
            made[fence].append(e)
    yield made
    for pair in made.values():
        for e in pair:
            e.close()


_BASE, _WANT = {}, {}


def _base(engines):
    """``base`` of session_model.expected: the plain progressive RGB session on the second engine, cached by its inputs -> frames; the cuts
    it reported are left in ``base.cuts``"""
    def base(brow, frames, marks):
        h = frames[0].shape[0]
        digest = hashlib.sha1(b"".join(np.ascontiguousarray(f).tobytes() for f in frames)).hexdigest()
        key = (brow, h, digest, marks)
        if key not in _BASE:
            with M.RawSession(engines[brow.fence][1], brow.batch, h) as s:
                assert s.configure(brow) == 0
                got, cuts = s.run(frames, marks[0] if marks else None)
            assert [i for i, _ in got] == list(range(len(frames)))
            _BASE[key] = ([f for _, f in got], cuts)
        base.cuts = _BASE[key][1]
        return _BASE[key][0]
    return base


def _want(row, engines):
    """(the frames a session of ``row`` must deliver, the cuts it must report): computed once, shared by A, B and C, never changed"""
    if row not in _WANT:
        base = _base(engines)
        want = M.expected(row, M.pushed_frames(row), base)
        for _, f in want:
            f.setflags(write=False)
        if row.scenes != "off":
            assert base.cuts, f"the plain session reports no cut: scenes are not live in {row}"
        _WANT[row] = (want, list(base.cuts) if row.scenes != "off" else [])
    return _WANT[row]


def _same(got, want, row, where):
    gi, wi = [i for i, _ in got[0]], [i for i, _ in want[0]]
    assert gi == wi, f"{where}: delivered indices {gi}, expected {wi}\n{_show(row)}"
    for (i, a), (_, b) in zip(got[0], want[0]):
        assert a.dtype == b.dtype and a.shape == b.shape, f"{where}: frame {i} is {a.dtype} {a.shape}, expected {b.dtype} {b.shape}\n{_show(row)}"
        if not np.array_equal(a, b):
            raise AssertionError(f"{where}: frame {i} differs in {int((a != b).sum())} of {a.size} samples\n{_show(row)}")
    assert got[1] == want[1], f"{where}: cuts {got[1]}, expected {want[1]}\n{_show(row)}"


def _show(row):
    return "\n".join(f"    {f} = {row.get(f)!r}" for f in M.FACTORS)


def _sequence(s, row):
    return s.run(M.pushed_frames(row), M.CUT if row.scenes == "manual" else None)


def _fresh(engines, row):
    with M.RawSession(engines[row.fence][0], row.batch) as s:
        assert s.configure(row) == 0, "a freshly opened session takes its setters in VideoStream's order"
        return _sequence(s, row)


# ---- the factors are live -------------------------------------------------------------------------------------------------------------------
def test_the_fence_weights_leave_the_range(engines):
    x = np.stack([f.astype(np.float32) / 255. for f in M.content(8)])
    eng = engines[True][1]
    was = eng.range_reruns()
    y = eng.forward(np.ascontiguousarray(PM.sliding_windows(x, M.T)[:1]))       # a host-pointer call reruns by itself
    assert np.isfinite(y).all() and eng.range_reruns() == was + 1
    eng = engines[False][1]
    was = eng.range_reruns()
    eng.forward(np.ascontiguousarray(PM.sliding_windows(x, M.T)[:1]))
    assert eng.range_reruns() == was


# ---- A. fresh sessions ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(FRESH)))
def test_a_fresh_session_delivers_the_models_bytes(engines, k):
    for n, row in enumerate(FRESH[k]):
        _same(_fresh(engines, row), _want(row, engines), row, f"row {16 * k + n}")


# ---- B. one session, walked -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(WALKS)))
def test_one_session_walked_through_the_rows(engines, k):
    order, (fence, batch), ahead, rows, step = WALKS[k]
    home = M.with_(M.DEFAULT, fence=fence, batch=batch)
    with M.RawSession(engines[fence][0], batch) as s:
        if ahead is not None:                                            # the predecessor of this chunk's first row, as in one long walk
            s.configure(ahead)
            _same(_sequence(s, ahead), _want(ahead, engines), ahead, f"{order} walk, the row ahead of step {step}")
        for n, row in enumerate(rows):
            if (step + n) % 4 == 3:                                      # the reconfiguration meets work in flight
                s.abandon(M.pushed_frames(s.row))
                s.reset()
            s.configure(row)
            _same(_sequence(s, row), _want(row, engines), row, f"{order} walk of {(fence, batch)}, step {step + n}")
        s.configure(home)                                                # ... and what a freshly opened session delivers
        _same(_sequence(s, home), _want(home, engines), home, f"{order} walk of {(fence, batch)}, back at the defaults")


# ---- C. refusals leave no trace -------------------------------------------------------------------------------------------------------------
REFUSED = ROWS[::len(ROWS) // 20][:20]


def _refusal(s, row, turn):
    """(the setter call ``row``'s setting must refuse, words of its answer): the first kind, from ``turn`` on, that applies to the row; each
    is a change after which session_model.legal says no"""
    pf, depth, chroma, pack = row.in_
    of, out_chroma, out_pack = row.out
    a = M.arguments(row)
    lib = s.lib
    for kind in (turn % 3, (turn + 1) % 3, (turn + 2) % 3):
        if kind == 0 and of in _capi.FORMATS_420 and out_chroma != "444":
            assert not M.legal(M.with_(row, size="odd"))
            return (lambda: lib.pfnl_stream_resize(s.s, 37, 55)), ("even output size" if out_chroma == "420" else "even output width")
        if kind == 1 and pf != "rgb24":
            assert not M.legal(M.with_(row, out=("rgb10", "420", None)))
            return ((lambda: lib.pfnl_stream_format(s.s, a["format"][0], _capi.PIXEL_FORMATS["rgb10"], *a["format"][2:])),
                    "PFNL_PIX_RGB10 is delivered for RGB24 input only")
        if kind == 2:
            wrong = "yuyv422" if pf == "rgb24" else "bgra"
            assert not M.legal(M.with_(row, in_=(pf, depth, chroma, wrong)))
            return ((lambda: lib.pfnl_stream_packing(s.s, _capi.PACKINGS[wrong], a["packing"][1])),
                    "input packing: a YUV packing" if pf == "rgb24" else "input packing: an RGB packing")
    raise AssertionError("the packing of the wrong family applies to every row")


@pytest.mark.parametrize("k", range(len(REFUSED)))
def test_a_refused_call_leaves_no_trace(engines, k):
    row = REFUSED[k]
    with M.RawSession(engines[row.fence][0], row.batch) as s:
        s.configure(row)
        call, words = _refusal(s, row, k)
        assert call() == M.INVALID and words in s.error(), s.error()
        _same(_sequence(s, row), _want(row, engines), row, f"row {ROWS.index(row)} behind a refused call")


def test_refused_interlacing_leaves_no_trace(engines):
    """4:2:0 planes of 18 rows: H % 4 != 0 is out of reach at H = 16, so this session has frames of 18 x 24"""
    h = 18
    row = M.with_(M.DEFAULT, in_=("i420", 8, "420", None))
    with pytest.raises(ValueError):
        M.arguments(M.with_(row, interlace=("frame", "tff")), h)
    pushed = M.pushed_frames(row, h)
    want = M.expected(row, pushed, _base(engines), h)
    with M.RawSession(engines[False][0], 1, h) as s:
        s.configure(row)
        assert s.lib.pfnl_stream_interlace(s.s, 1, 0) == M.INVALID and "multiple of 4" in s.error(), s.error()
        _same(s.run(pushed), (want, []), row, "18 x 24 behind refused interlacing")
