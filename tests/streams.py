"""Helpers of the stream-contract tests (tests/test_gpu_streams.py; DESIGN.md "What a call is ordered with").

Every entry of the library that takes a stream is "asynchronous on `stream`".  On the legacy null stream that claim cannot fail: the null
stream synchronises implicitly with every blocking stream, the handle's own among them.  The tests here run the library where that
implicit ordering is gone - on a hipStreamNonBlocking stream S, as a decode -> SR -> encode pipeline does - and make a mis-ordered step
visible with a delay:

* Probe L ("late input"): the input buffers hold a completed fill (quiet NaN, 0xA5 bytes).  On S: a spin kernel of D ms, the copy of
  the real input, the call, the copy of its result to pinned host memory.  Whatever part of the call runs ahead of S reads the fill.
* Probe N ("null stream asleep"): the null stream spins for D ms, then records e0.  On S, inputs complete: the call and the copy of its
  result.  After S.synchronize() the bits are right AND e0 has not completed: the call neither ran on nor waited for the null stream,
  nor for the handle's blocking stream, which waits behind it.

Both are preceded by an undelayed run of the same scenario on S (workspace, kernel attributes, torch's allocator, pinned buffers), whose
wall time sets D = max(25 ms, 3 x wall), capped at 250 ms.  D is the sensitivity, not a threshold; whether it is enough is what the two
CONTROLS say: an unordered plain copy must see the fill (L), a plain op on S must finish while the null stream still spins (N).  A probe
whose control does not hold FAILS ("insensitive on this device") - a probe that cannot fail is worse than none.

torch is imported where a function needs it: the module itself imports on a machine without it."""
from __future__ import annotations

import ctypes as C
import time
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np

D_MIN_MS, D_MAX_MS = 25.0, 250.0
CONTROL_D_MS = D_MIN_MS                           # the controls run at the smallest delay a probe can get
FILL = {1: 0xA5, 2: 0x7FC0, 4: 0x7FC00000, 8: 0x7FF8000000000000}   # per item size: bytes 0xA5; quiet NaN as bf16 / float32 / float64
HIP_STREAM_NON_BLOCKING = 0x01
MAX_EXPLICIT_TRIES = 4                            # one per hardware queue a process opens by default

_state: Dict[str, object] = {}


def delay_ms(warm_wall_ms: float) -> float:
    """D for a scenario whose undelayed warm-up took warm_wall_ms."""
    return float(min(D_MAX_MS, max(D_MIN_MS, 3.0 * warm_wall_ms)))


def fill_value(dtype_name: str, itemsize: int) -> int:
    """The fill of one element: integer types get 0xA5 bytes, floating types their quiet NaN."""
    if dtype_name.startswith(("uint", "int")):
        return int.from_bytes(bytes([0xA5]) * itemsize, "little")
    return FILL[itemsize]


def fill_like(a: np.ndarray) -> np.ndarray:
    """The fill pattern as a numpy array of a's shape and type (compared as bytes)."""
    v = fill_value(a.dtype.name, a.dtype.itemsize)
    return np.full(a.shape, v, dtype={1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]).view(a.dtype)


def same_bits(a: np.ndarray, b: np.ndarray) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


# ---------------------------------------------------------------------------------------------------------------------------------
# torch plumbing

_INT_VIEW = {1: "uint8", 2: "int16", 4: "int32", 8: "int64"}


def _as_int(t):
    """A flat integer view of a tensor: the types every copy and fill kernel knows (uint16 and bfloat16 go as int16)."""
    import torch
    return t.reshape(-1).view(getattr(torch, _INT_VIEW[t.element_size()]))


def fill_pattern(t) -> None:
    """The fill into a device tensor, on torch's current stream."""
    v = fill_value(str(t.dtype).replace("torch.", ""), t.element_size())
    bits = 8 * t.element_size()
    _as_int(t).fill_(v - (1 << bits) if t.element_size() > 1 and v >= 1 << (bits - 1) else v)


def to_device(a: np.ndarray):
    """A numpy array on the device, its type kept (uint16 through int16)."""
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)
    return torch.from_numpy(a).cuda()


def pinned_like(a: np.ndarray):
    """A pinned host tensor (integer view) holding a's bytes."""
    import torch
    a = np.ascontiguousarray(a).reshape(-1)
    return torch.from_numpy(a.view({1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize]).copy()).pin_memory()


def to_numpy(host_int, like) -> np.ndarray:
    """The bytes of a host tensor (as _as_int made it) in the shape and numpy type of the device tensor `like`."""
    name = str(like.dtype).replace("torch.", "")
    dt = {"bfloat16": np.uint16}.get(name) or np.dtype(name)
    return host_int.numpy().view(dt).reshape(tuple(like.shape)).copy()


def _hip():
    """The libamdhip64 this process (torch) has loaded already."""
    if "hip" not in _state:
        path = None
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64" in line:
                    path = line.split()[-1]
                    break
        assert path, "no libamdhip64 is loaded: import torch and initialise the device first"
        _state["hip"] = C.CDLL(path)
    return _state["hip"]


def _explicit_stream():
    """One hipStreamCreateWithFlags(hipStreamNonBlocking) stream as a torch ExternalStream; destroyed by teardown()."""
    import torch
    s = C.c_void_p()
    err = _hip().hipStreamCreateWithFlags(C.byref(s), C.c_uint(HIP_STREAM_NON_BLOCKING))
    assert err == 0 and s.value, f"hipStreamCreateWithFlags: {err}"
    _state.setdefault("explicit", []).append(s.value)
    return torch.cuda.ExternalStream(s.value)


def _destroy(stream) -> None:
    raw = stream.cuda_stream
    if raw in _state.get("explicit", []):
        _state["explicit"].remove(raw)
        _hip().hipStreamDestroy(C.c_void_p(raw))


def teardown() -> None:
    """Destroys the explicit streams and forgets the calibration and the controls' outcome."""
    import torch
    torch.cuda.synchronize()
    for raw in list(_state.get("explicit", [])):
        _hip().hipStreamDestroy(C.c_void_p(raw))
    hip = _state.get("hip")
    _state.clear()
    if hip is not None:
        _state["hip"] = hip


# ---------------------------------------------------------------------------------------------------------------------------------
# the delay

SPIN_CYCLES = 20_000_000


def _cycles_per_ms() -> float:
    """torch.cuda._sleep's cycles per millisecond: one fixed spin timed with events on an idle device, once per process."""
    if "cpm" not in _state:
        import torch
        torch.cuda._sleep(1000)                                               # (loads the kernel)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(SPIN_CYCLES)
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        assert ms > 0.05, f"the spin of {SPIN_CYCLES} cycles took {ms} ms: no delay can be built from it"
        _state["cpm"] = SPIN_CYCLES / ms
    return _state["cpm"]


def sleep_ms(ms: float) -> None:
    """Delays torch's current stream by ms milliseconds with a spin kernel of one wave: it holds a stream back without filling the GPU."""
    import torch
    torch.cuda._sleep(int(ms * _cycles_per_ms()))


# ---------------------------------------------------------------------------------------------------------------------------------
# the controls and the side streams

CONTROL_ELEMS = 1 << 16


def control_late(S, other=None, D: float = CONTROL_D_MS) -> bool:
    """Control L: on S a spin of D ms, then the copy of the real input over a completed fill.  A plain torch copy of that buffer issued
    on `other` (None: the null stream) without any ordering must see the fill - and the buffer holds the input in the end."""
    import torch
    _cycles_per_ms()
    real = np.arange(CONTROL_ELEMS, dtype=np.float32)
    buf = torch.empty(CONTROL_ELEMS, dtype=torch.float32, device="cuda")
    snap = torch.zeros(CONTROL_ELEMS, dtype=torch.float32, device="cuda")
    pin = pinned_like(real)
    fill_pattern(buf)
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        sleep_ms(D)
        _as_int(buf).copy_(pin, non_blocking=True)
    with torch.cuda.stream(other if other is not None else torch.cuda.default_stream()):
        snap.copy_(buf, non_blocking=True)
    torch.cuda.synchronize()
    return same_bits(snap.cpu().numpy(), fill_like(real)) and same_bits(buf.cpu().numpy(), real)


def control_null_asleep(S, D: float = CONTROL_D_MS) -> bool:
    """Control N: the null stream spins for D ms and records e0; a plain torch op on S completes, and S.synchronize() returns, while
    e0 is still pending."""
    import torch
    _cycles_per_ms()
    buf = torch.zeros(CONTROL_ELEMS, dtype=torch.float32, device="cuda")
    e0 = torch.cuda.Event()
    torch.cuda.synchronize()
    sleep_ms(D)
    e0.record()
    with torch.cuda.stream(S):
        buf.add_(1.0)
    S.synchronize()
    pending = not e0.query()
    torch.cuda.synchronize()
    return pending and bool((buf == 1.0).all())


def _both_controls(s) -> str:
    """"" when both null-stream controls hold on s, else which of them does not."""
    late, asleep = control_late(s), control_null_asleep(s)
    return "" if late and asleep else "L %s, N %s" % ("holds" if late else "fails", "holds" if asleep else "fails")


def _find_stream():
    """A stream both null-stream controls hold on: torch's pool first; where a pool stream shares its hardware queue with the null stream
    (the spin of one then delays the other), streams of our own, one per hardware queue at the most - a rejected one stays alive until
    the search ends, so that the next is placed on another queue.  (stream, how) or (None, why)."""
    import torch
    s = torch.cuda.Stream()
    why = _both_controls(s)
    if not why:
        return s, "torch.cuda.Stream()"
    tried, rejected, found = ["pool stream: " + why], [], None
    for k in range(MAX_EXPLICIT_TRIES):
        s = _explicit_stream()
        why = _both_controls(s)
        if not why:
            found = (s, f"hipStreamCreateWithFlags(hipStreamNonBlocking), attempt {k + 1} ({'; '.join(tried)})")
            break
        rejected.append(s)
        tried.append(f"explicit stream {k + 1}: {why}")
    for s in rejected:
        _destroy(s)
    return found or (None, "no stream passed (" + "; ".join(tried) + ")")


def keep_a_stream_alive() -> None:
    """One more explicit non-blocking stream that has run something and lives until teardown(): it takes the place the runtime would give
    the next stream a library creates (a session's copy stream), which then lands on another hardware queue."""
    import torch
    s = _explicit_stream()
    with torch.cuda.stream(s):
        torch.zeros(16, device="cuda").add_(1.0)
    s.synchronize()
    _state.setdefault("kept", []).append(s)


def sensitivity() -> Dict[str, object]:
    """Runs the controls once per process and picks the side streams by them.
    "S", "S2": the streams (None: none found); "L", "N": the null-stream forms of the two controls on S; "L2": the same two on S2;
    "pair": Control L with the unordered copy issued on S2; "how": a line for the report."""
    if "sens" not in _state:
        S, how = _find_stream()
        out: Dict[str, object] = {"S": S, "L": S is not None, "N": S is not None, "how": "S: " + how}
        if S is None:                                                         # say which of the two fails on a pool stream
            import torch
            p = torch.cuda.Stream()
            out["L"], out["N"] = control_late(p), control_null_asleep(p)
        S2, how2 = _find_stream()
        out.update(S2=S2, L2=S2 is not None, how=out["how"] + "; S2: " + how2)
        out["pair"] = bool(S is not None and S2 is not None and control_late(S, other=S2))
        _state["sens"] = out
    return _state["sens"]


def side_stream(second: bool = False):
    """The non-blocking stream the probes run on, usable as torch's current stream (second: the one a second handle runs on)."""
    sens = sensitivity()
    s = sens["S2" if second else "S"]
    assert s is not None, f"insensitive on this device: no side stream passes the controls ({sens['how']})"
    return s


def require(kind: str) -> None:
    """A probe of `kind` ("L" | "N" | "L2") means something on this device only if its control held."""
    sens = sensitivity()
    assert sens[kind], f"probe {kind}: insensitive on this device ({sens['how']})"


# ---------------------------------------------------------------------------------------------------------------------------------
# the probes

class Probe:
    """One scenario on a side stream.  inputs: the real inputs (numpy); body(device inputs) -> the results, a list of device tensors
    (copied to pinned host memory on S) and / or numpy arrays (what a host-pointer call returned), run with S as torch's current stream.
    owned: device tensors the scenario writes and the test owns - filled with the pattern before every run."""

    def __init__(self, label: str, S, inputs: Sequence[np.ndarray], body: Callable[[List[object]], List[object]], owned: Sequence[object] = (),
                 kind: str = "L"):
        import torch
        self.label, self.S, self.body, self.owned, self.kind = label, S, body, list(owned), kind
        self.inputs = [np.ascontiguousarray(a) for a in inputs]
        self.bufs = [to_device(fill_like(a)) for a in self.inputs]
        self.pins = [pinned_like(a) for a in self.inputs]
        self.host: List[object] = []
        self.D = None
        torch.cuda.synchronize()

    def _reset(self, real_inputs: bool) -> None:
        import torch
        for b, p in zip(self.bufs, self.pins):
            if real_inputs:
                _as_int(b).copy_(p)
            else:
                fill_pattern(b)
        for t in self.owned:
            fill_pattern(t)
        torch.cuda.synchronize()

    def _collect(self, res) -> List[np.ndarray]:
        """(on S) device results -> pinned host memory, allocated by the first run and reused"""
        import torch
        out = []
        for i, r in enumerate(res):
            if isinstance(r, np.ndarray):
                out.append((None, r))
                continue
            ri = _as_int(r)
            while len(self.host) <= i:
                self.host.append(None)
            if self.host[i] is None or self.host[i].shape != ri.shape or self.host[i].dtype != ri.dtype:
                self.host[i] = torch.empty(ri.shape, dtype=ri.dtype).pin_memory()
            self.host[i].copy_(ri, non_blocking=True)
            out.append((self.host[i], r))
        return out

    @staticmethod
    def _finish(pairs) -> List[np.ndarray]:
        return [r if h is None else to_numpy(h, r) for h, r in pairs]

    def warm_up(self) -> List[np.ndarray]:
        """The undelayed run on S; sets D from its wall time."""
        import torch
        self._reset(real_inputs=False)
        t0 = time.perf_counter()
        with torch.cuda.stream(self.S):
            for b, p in zip(self.bufs, self.pins):
                _as_int(b).copy_(p, non_blocking=True)
            pairs = self._collect(self.body(self.bufs))
        self.S.synchronize()
        self.D = delay_ms((time.perf_counter() - t0) * 1e3)
        out = self._finish(pairs)
        del pairs
        return out

    def enqueue_late(self) -> None:
        """Probe L, enqueued and not waited for: the spin, the late copy of the inputs, the call, the copy of its results."""
        import torch
        require(self.kind)
        assert self.D is not None, "warm_up() first"
        self._reset(real_inputs=False)
        with torch.cuda.stream(self.S):
            sleep_ms(self.D)
            for b, p in zip(self.bufs, self.pins):
                _as_int(b).copy_(p, non_blocking=True)
            self._pending = self._collect(self.body(self.bufs))

    def finish(self) -> List[np.ndarray]:
        self.S.synchronize()
        out = self._finish(self._pending)
        self._pending = None
        return out

    def late(self) -> List[np.ndarray]:
        """Probe L."""
        self.enqueue_late()
        return self.finish()

    def null_asleep(self):
        """Probe N: (results, e0 still pending after S.synchronize())."""
        import torch
        require("N")
        assert self.D is not None, "warm_up() first"
        self._reset(real_inputs=True)
        e0 = torch.cuda.Event()
        sleep_ms(self.D)                                                       # (torch's current stream here: the null stream)
        e0.record()
        with torch.cuda.stream(self.S):
            pairs = self._collect(self.body(self.bufs))
        self.S.synchronize()
        pending = not e0.query()
        torch.cuda.synchronize()
        out = self._finish(pairs)
        del pairs
        return out, pending


def report(scenario: str, probe: str, D: Optional[float], verdict: str, extra: str = "") -> None:
    d = "D = %5.1f ms" % D if D is not None else "D =   -     "
    print(f"\n[streams] {scenario:58s} {probe:12s} {d}  {verdict}  {extra}", end="")
