"""Helpers of the host-thread tests (tests/test_gpu_threads.py; host tests of these helpers: tests/test_threads_host.py; DESIGN.md "What
handles share").

include/pfnl_hip.h: "A handle is bound to one device and is not re-entrant; distinct handles are independent."  The tests run distinct
handles from distinct host threads AT THE SAME MOMENT and compare every result bit for bit with the one the same handle computed alone.

* run_together: one Python thread per worker, a barrier ahead of every round so that the round's calls start together (ctypes releases
  the GIL inside a library call).  Trouble ends the run: the first exception breaks the barrier and is raised on the calling thread with
  its worker's name and round; a worker still alive at the time limit is reported by name, round and last stamp.  Nothing is retried.
* overlap_share: the share of rounds in which at least two workers' calls really overlapped.  A concurrency test whose calls ran one after
  another shows nothing and is worse than none: below one half it FAILS as insensitive (require_overlap), as the controls of
  tests/streams.py do.  One half is a condition, not a measurement: every call of the GPU tests is a whole forward or more (>= 0.4 ms),
  against a barrier release of tens of microseconds.

The module needs neither torch nor a device."""
from __future__ import annotations

import threading
import time
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Sequence, Tuple

import history as Hy

ROUNDS = 6
MAX_WORKERS = 4
MIN_SHARE = 0.5
GRACE_S = 2.0                                     # for the workers an aborted barrier has released to end, once the time limit has passed

# part A of tests/test_gpu_threads.py: three groups of four trunk families (history.FAMILIES) that hold every pair of the six
GROUPS_A: Tuple[Tuple[str, ...], ...] = (("small", "mid", "chain", "chain_split"),
                                         ("small", "mid", "strict", "bf16"),
                                         ("chain", "chain_split", "strict", "bf16"))


def pairs_covered(groups: Sequence[Sequence[str]] = GROUPS_A) -> set:
    return {frozenset((a, b)) for g in groups for a in g for b in g if a != b}


def all_pairs(families: Sequence[str] = Hy.FAMILIES) -> set:
    return {frozenset((a, b)) for a in families for b in families if a != b}


def hang_guard_s(serial_wall_s: float) -> float:
    """run_together's time limit for a test whose serial pass took serial_wall_s: a hang guard measured against the serial run (50 x, at
    least a minute), not a speed claim."""
    return max(60.0, 50.0 * serial_wall_s)


class WorkerError(RuntimeError):
    """A worker raised: its name and round; the exception itself is __cause__."""

    def __init__(self, name: str, round_: int, exc: BaseException):
        super().__init__(f"worker {name!r}, round {round_}: {type(exc).__name__}: {exc}")
        self.name, self.round, self.exc = name, round_, exc


class WorkersStuck(RuntimeError):
    """Workers still alive at the time limit: [(name, round, seconds since their last stamp, inside a call?)]."""

    def __init__(self, stuck: List[Tuple[str, int, float, bool]], timeout_s: float):
        lines = [f"worker {n!r}, round {r}: {'inside its call' if busy else 'between calls'}, last stamp {age:.1f} s ago" for n, r, age, busy in stuck]
        super().__init__(f"still alive after {timeout_s:.1f} s: " + "; ".join(lines))
        self.stuck = stuck


@dataclass
class Run:
    names: List[str]
    results: Dict[str, List[object]] = field(default_factory=dict)              # name -> the result of every finished round, in order
    stamps: Dict[str, List[Tuple[float, float]]] = field(default_factory=dict)  # name -> (perf_counter before, after) of every finished round
    wall_s: float = 0.0

    def share(self) -> float:
        return overlap_share(self.stamps)


def run_together(workers, rounds: int = ROUNDS, timeout_s: float = 60.0) -> Run:
    """workers: {name: callable(round) -> result} (or a sequence of (name, callable)), `rounds` rounds of all of them at once.  Returns the
    Run when every worker finished every round; raises WorkerError for the first exception (the other workers stop at their next
    barrier) and WorkersStuck at the time limit.  The threads are daemons: a worker that never returns does not keep the process."""
    items = list(workers.items()) if isinstance(workers, dict) else list(workers)
    names = [n for n, _ in items]
    assert len(set(names)) == len(names) and 1 <= len(names), names
    run = Run(names, {n: [] for n in names}, {n: [] for n in names})
    barrier = threading.Barrier(len(items))
    lock = threading.Lock()
    errors: List[WorkerError] = []
    state: Dict[str, Tuple[int, float, bool]] = {n: (0, time.perf_counter(), False) for n in names}   # round, last stamp, inside the call

    def loop(name: str, fn: Callable[[int], object]) -> None:
        for r in range(rounds):
            try:
                barrier.wait()
            except threading.BrokenBarrierError:
                return
            t0 = time.perf_counter()
            state[name] = (r, t0, True)
            try:
                res = fn(r)
            except BaseException as e:  # noqa: BLE001   (whatever it is, it ends the run and is raised on the main thread)
                with lock:
                    errors.append(WorkerError(name, r, e))
                state[name] = (r, time.perf_counter(), False)
                barrier.abort()
                return
            t1 = time.perf_counter()
            run.results[name].append(res)
            run.stamps[name].append((t0, t1))
            state[name] = (r, t1, False)

    threads = [threading.Thread(target=loop, args=item, name=f"worker-{item[0]}", daemon=True) for item in items]
    began = time.perf_counter()
    for t in threads:
        t.start()
    deadline = time.monotonic() + timeout_s
    for t in threads:
        t.join(max(0.0, deadline - time.monotonic()))
    run.wall_s = time.perf_counter() - began
    alive = [t for t in threads if t.is_alive()]
    if alive:
        barrier.abort()                                                           # no further round starts
        busy = {n: state[n] for n in names}                                       # (as they were at the limit)
        end = time.monotonic() + GRACE_S
        for t in alive:
            if not busy[t.name[len("worker-"):]][2]:                              # parked at the barrier: released by the abort
                t.join(max(0.0, end - time.monotonic()))
    if errors:
        raise errors[0] from errors[0].exc
    if alive:
        now = time.perf_counter()
        late = [t.name[len("worker-"):] for t in alive]
        late = [n for n in late if busy[n][2]] or late                            # those inside a call; none: whoever had not finished
        raise WorkersStuck([(n, busy[n][0], now - busy[n][1], busy[n][2]) for n in late], timeout_s)
    return run


def overlap_share(stamps: Dict[str, Sequence[Tuple[float, float]]]) -> float:
    """The share of rounds in which at least two workers' call intervals intersect (touching ends do not).  A round counts once any
    worker has stamps for it; no rounds at all: 0."""
    rounds = max((len(v) for v in stamps.values()), default=0)
    if not rounds:
        return 0.0
    hit = 0
    for r in range(rounds):
        iv = sorted(v[r] for v in stamps.values() if len(v) > r)
        # sorted by start: two intervals intersect iff some interval starts before the latest end seen so far
        latest, found = None, False
        for a, b in iv:
            if latest is not None and a < latest:
                found = True
                break
            latest = b if latest is None else max(latest, b)
        hit += found
    return hit / rounds


def require_overlap(label: str, run: Run, serial_wall_s: float, extra: str = "") -> float:
    """Prints the test's line (pytest -s) and fails it as insensitive below MIN_SHARE."""
    share = run.share()
    print(f"\n[threads] {label:44s} {len(run.names)} workers x {max(len(v) for v in run.stamps.values())} rounds  overlap share {share:.2f}  "
          f"serial pass {serial_wall_s * 1e3:8.1f} ms  together {run.wall_s * 1e3:8.1f} ms  {extra}", end="")
    assert share >= MIN_SHARE, f"{label}: insensitive - the calls of {share:.2f} of the rounds overlapped, {MIN_SHARE} are required"
    return share


def timed(fn: Callable[[], object]) -> Tuple[object, float]:
    t0 = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t0
