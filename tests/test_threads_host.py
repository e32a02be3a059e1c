"""Host tests of tests/threads.py with stub workers: no device, no torch."""
import threading
import time

import pytest

import history as Hy
import threads as Th


def test_results_arrive_per_worker_and_in_round_order():
    seen = []
    workers = {name: (lambda r, name=name: (seen.append((name, r)), (name, r * r))[1]) for name in ("a", "b", "c")}
    run = Th.run_together(workers, rounds=5, timeout_s=30.0)
    assert run.names == ["a", "b", "c"]
    for name in run.names:
        assert run.results[name] == [(name, r * r) for r in range(5)]
        assert len(run.stamps[name]) == 5 and all(t0 <= t1 for t0, t1 in run.stamps[name])
        assert all(run.stamps[name][r][1] <= run.stamps[name][r + 1][0] for r in range(4))
    # the barrier: no worker begins round r + 1 before every worker has begun round r
    for r in range(4):
        assert max(seen.index((n, r)) for n in run.names) < min(seen.index((n, r + 1)) for n in run.names)


def test_a_barrier_holds_every_round_back_until_all_have_finished_the_one_before():
    ends = {}

    def slow(r):
        time.sleep(0.02)
        ends[r] = time.perf_counter()

    run = Th.run_together({"slow": slow, "quick": lambda r: None}, rounds=3, timeout_s=30.0)
    for r in range(1, 3):
        assert run.stamps["quick"][r][0] >= ends[r - 1]


def test_an_exception_surfaces_with_its_workers_name_and_the_others_end():
    calls = {"good": 0, "other": 0}

    def bad(r):
        if r == 2:
            raise ValueError("status 7")
        return r

    def counting(name):
        def fn(r):
            calls[name] += 1
            return r
        return fn

    before = threading.active_count()
    with pytest.raises(Th.WorkerError, match=r"worker 'bad', round 2: ValueError: status 7") as ei:
        Th.run_together({"good": counting("good"), "bad": bad, "other": counting("other")}, rounds=6, timeout_s=30.0)
    assert ei.value.name == "bad" and ei.value.round == 2 and isinstance(ei.value.__cause__, ValueError)
    # no round 3 began (round 2: a worker the abort catches while it is still leaving the barrier ends without its call)
    assert all(c in (2, 3) for c in calls.values()), calls
    assert threading.active_count() == before                                      # every worker has ended


def test_a_parked_worker_is_reported_at_the_time_limit():
    gate = threading.Event()
    calls = []

    def parked(r):
        if r == 1:
            gate.wait()
        return r

    t0 = time.perf_counter()
    try:
        with pytest.raises(Th.WorkersStuck, match=r"worker 'parked', round 1: inside its call") as ei:
            Th.run_together({"parked": parked, "free": lambda r: calls.append(r)}, rounds=4, timeout_s=0.3)
        took = time.perf_counter() - t0
        assert [(n, r, busy) for n, r, _, busy in ei.value.stuck] == [("parked", 1, True)]
        assert ei.value.stuck[0][2] >= 0.2                                          # seconds since the stamp ahead of its call
        assert took < 0.3 + Th.GRACE_S + 5.0                                        # pytest did not hang on it
        assert calls == [0, 1]                                                      # no further round started
    finally:
        gate.set()


@pytest.mark.parametrize("stamps,share", [
    ({"a": [(0.0, 1.0)], "b": [(2.0, 3.0)]}, 0.0),                                  # disjoint
    ({"a": [(0.0, 4.0)], "b": [(1.0, 2.0)]}, 1.0),                                  # nested
    ({"a": [(0.0, 1.0)], "b": [(1.0, 2.0)]}, 0.0),                                  # touching
    ({"a": [(0.0, 1.0)], "b": [(2.0, 3.0)], "c": [(2.5, 2.6)]}, 1.0),               # two of three
    ({"a": [(0.0, 1.0), (5.0, 6.0)], "b": [(0.5, 2.0), (6.5, 7.0)]}, 0.5),          # one round of two
    ({"a": [(0.0, 1.0)]}, 0.0),                                                     # one worker
    ({}, 0.0), ({"a": []}, 0.0),
])
def test_overlap_share_on_literal_intervals(stamps, share):
    assert Th.overlap_share(stamps) == share


def test_sleeping_workers_reach_a_share_of_one():
    run = Th.run_together({n: (lambda r: time.sleep(0.02)) for n in ("a", "b", "c")}, rounds=4, timeout_s=30.0)
    assert run.share() == 1.0
    assert Th.require_overlap("stub sleepers", run, 0.0) == 1.0


def test_serial_calls_fail_as_insensitive():
    run = Th.Run(["a", "b"], {"a": [0], "b": [0]}, {"a": [(0.0, 1.0)], "b": [(1.5, 2.5)]})
    with pytest.raises(AssertionError, match="insensitive"):
        Th.require_overlap("one after another", run, 0.0)


def test_the_hang_guard_is_fifty_serial_passes_and_at_least_a_minute():
    assert Th.hang_guard_s(0.1) == 60.0 and Th.hang_guard_s(3.0) == 150.0


def test_the_groups_of_part_a_cover_all_15_pairs():
    assert len(Hy.FAMILIES) == 6 and len(Th.all_pairs()) == 15
    assert all(len(g) == Th.MAX_WORKERS and set(g) <= set(Hy.FAMILIES) for g in Th.GROUPS_A)
    assert Th.pairs_covered() == Th.all_pairs()
    assert [t.family for t in Hy.family_targets()] == list(Hy.FAMILIES)
