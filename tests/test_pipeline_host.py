"""graphchainer_amd.pipeline with fake stages: order, the bound on items between source and sink, lazy workers, two replicas, a failure in each stage, and the
out-of-memory retirement. No device and no library: the stages are callables of this file. Every run goes through run_with_timeout, which fails instead of hanging."""
import random
import threading
import time

import pytest

from graphchainer_amd import pipeline

JOIN_SECONDS = 20


def run_with_timeout(**kw):
    """pipeline.run on a thread of its own, joined with a timeout: -> (report or None, exception or None)."""
    box = {}

    def target():
        try:
            box["report"] = pipeline.run(**kw)
        except BaseException as e:   # noqa: B036 - handed to the test
            box["error"] = e

    t = threading.Thread(target=target, daemon=True)
    t.start()
    t.join(JOIN_SECONDS)
    assert not t.is_alive(), "the pipeline did not end within its timeout"
    return box.get("report"), box.get("error")


class Worker:
    """What a factory makes: remembers its replica, the items it worked on, and whether it was closed."""

    def __init__(self, log, replica):
        self.replica, self.items, self.closed = replica, [], 0
        self.number = len(log)
        log.append(self)

    def close(self):
        self.closed += 1


def simple_source(n):
    def source(choose):
        for i in range(n):
            choose()
            yield i
    return source


def uneven_times(n, seed=5):
    rng = random.Random(seed)
    return [rng.uniform(0.2, 1.0) * 0.006 * (n - i) / n for i in range(n)]   # the later items are the faster ones: they overtake the earlier


@pytest.mark.parametrize("workers", [1, 3, 5])
def test_results_reach_the_sink_in_input_order(workers):
    n, times, made, got = 40, uneven_times(40), [], []
    finished = []

    def work(obj, replica, item):
        time.sleep(times[item])
        obj.items.append(item)
        finished.append(item)
        return item, item * item + 1

    report, error = run_with_timeout(source=simple_source(n), factory=lambda r: Worker(made, r), work=work, sink=got.append, inflight=workers)
    assert error is None
    assert got == [(i, i * i + 1) for i in range(n)]
    assert report["items"] == n and report["items_per_replica"] == [n] and report["retired_workers"] == 0
    assert 1 <= len(made) <= workers and report["workers_made"] == [len(made)]
    assert all(w.closed == 1 for w in made)
    assert sorted(i for w in made for i in w.items) == list(range(n))
    if workers > 1:
        assert finished != sorted(finished), "the fake work never finished out of order: the test shows nothing"
    stages = report["stage_seconds"]
    assert set(stages) == {"source", "work", "sink"} and all(set(s) == {"busy", "waiting_in", "waiting_out"} for s in stages.values())
    assert stages["work"]["busy"] >= 0.9 * sum(times)


@pytest.mark.parametrize("inflight", [1, 3])
def test_source_is_held_to_inflight_plus_two_ahead_of_the_sink(inflight):
    n, sunk, ahead, made = 30, [], [], []

    def source(choose):
        for i in range(n):
            choose()
            ahead.append(i + 1 - len(sunk))       # items begun, this one included, that the sink has not taken
            yield i

    def sink(result):
        time.sleep(0.003)                         # the slow end: the source would run away without the bound
        sunk.append(result)

    report, error = run_with_timeout(source=source, factory=lambda r: Worker(made, r), work=lambda o, r, i: i, sink=sink, inflight=inflight)
    assert error is None and sunk == list(range(n))
    assert max(ahead) <= inflight + 2
    assert max(ahead) == inflight + 2, "the bound was never reached: the test shows nothing"


def test_workers_are_made_lazily():
    made, got = [], []
    report, error = run_with_timeout(source=simple_source(2), factory=lambda r: Worker(made, r), work=lambda o, r, i: (time.sleep(0.02), i)[1], sink=got.append, inflight=5)
    assert error is None and got == [0, 1]
    assert 1 <= len(made) <= 2 and report["workers_made"] == [len(made)]

    made, got = [], []

    def slow_source(choose):
        for i in range(5):
            choose()
            time.sleep(0.03)                      # slower than the work: the one worker is idle again before the next item is ready
            yield i

    report, error = run_with_timeout(source=slow_source, factory=lambda r: Worker(made, r), work=lambda o, r, i: i, sink=got.append, inflight=5)
    assert error is None and got == list(range(5))
    assert len(made) == 1 and report["workers_made"] == [1]


def test_two_replicas_fewest_outstanding_then_round_robin():
    n, made, got, chosen = 8, [], [], []
    gate = threading.Event()

    def source(choose):
        for i in range(n):
            chosen.append(choose())
            assert choose() == chosen[-1]         # asked again before the yield: the same answer
            yield i
        gate.set()

    def work(obj, replica, item):
        gate.wait(JOIN_SECONDS)                   # nothing finishes while the source chooses: the choice is by count alone
        assert obj.replica == replica
        obj.items.append(item)
        return item, replica

    report, error = run_with_timeout(source=source, factory=lambda r: Worker(made, r), work=work, sink=got.append, replicas=2, inflight=3)
    assert error is None
    assert chosen == [0, 1, 0, 1, 0, 1, 0, 1]   # a tie every time: round-robin from the last one chosen
    assert got == [(i, chosen[i]) for i in range(n)]
    assert report["items_per_replica"] == [4, 4]
    for w in made:
        assert all(chosen[i] == w.replica for i in w.items) and w.closed == 1

    # uneven: both items of replica 0 end while replica 1's two are still at work, so the count, not the turn, decides
    made, got, chosen, released = [], [], [], []
    go, gate2 = threading.Event(), threading.Event()

    def source2(choose):
        for i in range(n):
            if i == 4:
                go.set()
                deadline = time.time() + JOIN_SECONDS
                while not {0, 2} <= set(released) and time.time() < deadline:     # released: their work is over and counted
                    time.sleep(0.001)
            chosen.append(choose())
            yield i
        gate2.set()

    def work2(obj, replica, item):
        (go if item in (0, 2) else gate2).wait(JOIN_SECONDS)
        return item, replica

    report, error = run_with_timeout(source=source2, factory=lambda r: Worker(made, r), work=work2, sink=got.append, replicas=2, inflight=4, release=released.append)
    assert error is None and [g[0] for g in got] == list(range(n))
    # item 4: 0 outstanding against 2; item 5: 1 against 2, where the turn alone would say replica 1; item 6: a tie, the turn; item 7: 2 against 3
    assert chosen == [0, 1, 0, 1, 0, 0, 1, 0]
    assert all(g[1] == chosen[g[0]] for g in got)
    assert report["items_per_replica"] == [5, 3]


class Boom(Exception):
    pass


def check_failure(kind):
    before = threading.active_count()
    n, made, got, released = 20, [], [], []

    def source(choose):
        for i in range(n):
            choose()
            if kind == "source" and i == 9:
                raise Boom("source")
            yield i

    def work(obj, replica, item):
        time.sleep(0.002 * (item % 3))
        if kind == "worker" and item == 7:
            raise Boom("worker")
        return item

    def sink(result):
        if kind == "sink" and result == 5:
            raise Boom("sink")
        got.append(result)

    report, error = run_with_timeout(source=source, factory=lambda r: Worker(made, r), work=work, sink=sink, inflight=3, release=released.append)
    assert report is None and isinstance(error, Boom) and str(error) == kind
    assert got == list(range(len(got))), "the sink saw a gap"
    assert len(got) <= {"source": 9, "worker": 7, "sink": 5}[kind]
    assert made and all(w.closed == 1 for w in made)
    assert sorted(released) == list(range(len(released))) and len(set(released)) == len(released)   # every item yielded was released once
    deadline = time.time() + JOIN_SECONDS
    while threading.active_count() > before and time.time() < deadline:
        time.sleep(0.01)
    assert threading.active_count() == before


def test_failure_in_the_source():
    check_failure("source")


def test_failure_in_a_worker():
    check_failure("worker")


def test_failure_in_the_sink():
    check_failure("sink")


def test_failure_inside_a_prefetched_iterator_and_its_thread_ends():
    before = threading.active_count()

    def pieces():
        yield b"a"
        yield b"b"
        raise Boom("reader")

    def source(choose):
        with pipeline.Prefetch(pieces()) as items:
            for piece in items:
                choose()
                yield piece

    got, made = [], []
    report, error = run_with_timeout(source=source, factory=lambda r: Worker(made, r), work=lambda o, r, i: i, sink=got.append, inflight=2)
    assert isinstance(error, Boom) and str(error) == "reader" and got in ([], [b"a"], [b"a", b"b"])
    assert threading.active_count() == before

    # and when a later stage fails, the reader thread is stopped although its iterator has more
    def endless():
        while True:
            yield b"x"

    def source2(choose):
        with pipeline.Prefetch(endless()) as items:
            for piece in items:
                choose()
                yield piece

    def sink(result):
        if len(got2) == 3:
            raise Boom("sink")
        got2.append(result)

    got2 = []
    report, error = run_with_timeout(source=source2, factory=lambda r: Worker(made, r), work=lambda o, r, i: i, sink=sink, inflight=2)
    assert isinstance(error, Boom) and str(error) == "sink" and got2 == [b"x"] * 3
    assert threading.active_count() == before


def test_out_of_memory_retires_a_worker_and_the_run_completes():
    n, made, got = 12, [], []
    both = threading.Barrier(2)

    def work(obj, replica, item):
        if not obj.items:
            both.wait(JOIN_SECONDS)               # the first call of each of the first two workers: both exist
        obj.items.append(item)
        if obj.number == 1 and len(obj.items) == 1:
            raise RuntimeError("hipMalloc failed: out of memory (asked for 3 GB)")
        time.sleep(0.001)
        return item

    report, error = run_with_timeout(source=simple_source(n), factory=lambda r: Worker(made, r), work=work, sink=got.append, inflight=2)
    assert error is None and got == list(range(n))
    assert report["retired_workers"] == 1 and report["limits"] == [1]
    assert len(made) == 2 and all(w.closed == 1 for w in made)
    assert made[1].items and len(made[1].items) == 1      # the retired worker took nothing more
    assert sorted(set(made[0].items)) == list(range(n))   # its item went to the other worker


def test_out_of_memory_in_the_only_worker_is_the_runs_error():
    made, got = [], []

    def work(obj, replica, item):
        if item == 2:
            raise RuntimeError("graphchainer_amd error 3: out of memory")
        return item

    report, error = run_with_timeout(source=simple_source(6), factory=lambda r: Worker(made, r), work=work, sink=got.append, inflight=1)
    assert isinstance(error, RuntimeError) and "out of memory" in str(error)
    assert got == list(range(len(got))) and len(got) <= 2     # (the failure stops the sink too: a prefix of what came before item 2)
    assert len(made) == 1 and made[0].closed == 1

    # a limit of 3 retires two workers at the most: the third failure is the run's
    made, got = [], []

    def always(obj, replica, item):
        raise RuntimeError("out of memory")

    report, error = run_with_timeout(source=simple_source(6), factory=lambda r: Worker(made, r), work=always, sink=got.append, inflight=3)
    assert isinstance(error, RuntimeError) and got == []
    assert len(made) == 3 and all(w.closed == 1 for w in made)


def test_arguments_are_checked_and_the_package_exports_the_module():
    import graphchainer_amd
    assert graphchainer_amd.pipeline is pipeline
    with pytest.raises(ValueError):
        pipeline.run(simple_source(1), lambda r: None, lambda o, r, i: i, lambda x: None, inflight=0)
    with pytest.raises(ValueError):
        pipeline.run(simple_source(1), lambda r: None, lambda o, r, i: i, lambda x: None, replicas=2, inflight=[1])
