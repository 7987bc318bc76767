"""An ordered pipeline of host threads: a source, up to `inflight` workers per replica, a sink that sees the results in input order.

It knows nothing of a device or of the library: every stage is a callable the caller brings, so the order, the bound, the lazy workers, the failure handling and the
out-of-memory retirement are tested on the CPU (tests/test_pipeline_host.py). The command line (cli.run) puts the read parser, one Aligner per worker and the output
writer behind it; a replica there is one device's copy of the graph and its index.

    report = run(source, factory, work, sink, replicas=2, inflight=3)

  source(choose)      generator function run on the source thread. Before it makes an item it calls choose() -> the replica the item will be worked on (the one with the
                      fewest items outstanding, ties broken round-robin from the last one chosen); choose() is also where the source waits while inflight_total + 2 items
                      exist between it and the sink. Then it yields the item. choose() twice without a yield between gives the same answer (a parse that found no record).
  factory(replica)    makes the object a worker thread owns (an Aligner); called on that thread, and only when an item is ready, every worker of the replica is busy and
                      fewer than its limit exist. Its close() is called on the same thread when the worker ends.
  work(obj, replica, item) -> result     on a worker thread.
  sink(result)        on the sink thread, strictly in the order the source yielded.
  release(item)       optional: called once for every item the source yielded, when its work is over or when a failed run drops it.

An exception in any stage stops the others; every worker object is closed, every thread joined, and the first exception is raised in the caller. A work() that fails
with a RuntimeError whose text holds "out of memory" while its replica may have more than one worker retires that worker instead: it is closed, the replica's limit drops
by one and the item goes back to the front of the replica's queue.
"""
import threading
import time
from collections import deque

__all__ = ["run", "Prefetch", "OUT_OF_MEMORY"]

OUT_OF_MEMORY = "out of memory"


class _Stopped(BaseException):
    """Raised inside a stage that waited while the run was stopped; never leaves this module."""


class Prefetch:
    """Runs an iterator one step ahead on a thread of its own (the file reader: read() and zlib release the GIL): `with Prefetch(it) as items: for x in items`.
    At most `depth` items wait and one is being made. An exception of the iterator is raised where the items are consumed. Leaving the block stops the thread, closes
    the iterator on it and joins it. busy / waiting_out: seconds inside the iterator / waiting for room; consumer_waiting: seconds the consumer waited for an item."""

    def __init__(self, iterator, depth=1, name="prefetch"):
        self.iterator, self.depth = iterator, max(1, depth)
        self.cond = threading.Condition()
        self.items, self.done, self.stop, self.error = deque(), False, False, None
        self.busy = self.waiting_out = self.consumer_waiting = 0.0
        self.thread = threading.Thread(target=self._produce, name=name, daemon=True)

    def _produce(self):
        try:
            while True:
                t0 = time.perf_counter()
                try:
                    item = next(self.iterator)
                except StopIteration:
                    break
                finally:
                    self.busy += time.perf_counter() - t0
                t0 = time.perf_counter()
                with self.cond:
                    while len(self.items) >= self.depth and not self.stop:
                        self.cond.wait()
                    self.waiting_out += time.perf_counter() - t0
                    if self.stop:
                        break
                    self.items.append(item)
                    self.cond.notify_all()
        except BaseException as e:   # noqa: B036 - handed to the consumer
            self.error = e
        finally:
            try:
                close = getattr(self.iterator, "close", None)
                if close is not None:
                    close()
            except BaseException as e:   # noqa: B036
                self.error = self.error or e
            with self.cond:
                self.done = True
                self.cond.notify_all()

    def __enter__(self):
        self.thread.start()
        return self

    def __iter__(self):
        return self

    def __next__(self):
        t0 = time.perf_counter()
        with self.cond:
            while not self.items and not self.done:
                self.cond.wait()
            self.consumer_waiting += time.perf_counter() - t0
            if self.items:
                item = self.items.popleft()
                self.cond.notify_all()
                return item
            if self.error is not None:
                error, self.error = self.error, None
                raise error
            raise StopIteration

    def __exit__(self, kind, value, trace):
        with self.cond:
            self.stop = True
            self.items.clear()
            self.cond.notify_all()
        if self.thread.ident is not None:
            self.thread.join()
        return False


class _Replica:
    def __init__(self, limit):
        self.limit = limit                 # workers this replica may have; drops by one per retirement
        self.queue = deque()               # (seq, item) ready for a worker
        self.workers = 0                   # worker threads alive (being made included)
        self.idle = 0                      # of them, waiting for an item
        self.outstanding = 0               # items chosen for this replica whose work is not over
        self.items = 0                     # items worked here
        self.made = 0                      # factory calls
        self.retired = 0


class _Run:
    def __init__(self, source, factory, work, sink, replicas, inflight, release):
        limits = list(inflight) if isinstance(inflight, (list, tuple)) else [inflight] * replicas
        if replicas < 1 or len(limits) != replicas or any(int(k) < 1 for k in limits):
            raise ValueError("replicas >= 1 and one inflight >= 1 per replica")
        self.source, self.factory, self.work, self.sink, self.release = source, factory, work, sink, release
        self.replicas = [_Replica(int(k)) for k in limits]
        self.slots = sum(int(k) for k in limits) + 2      # items between source and sink: every worker's, one parsed and waiting, one being parsed
        self.cond = threading.Condition()
        self.error = None                  # the first exception of any stage
        self.stopped = False
        self.alive = 0                     # items chosen (or yielded) and not yet through the sink
        self.produced = 0                  # items the source yielded
        self.source_done = False
        self.results = {}                  # seq -> result, until the sink takes it
        self.sunk = 0
        self.last_choice = -1
        self.threads = []
        self.seconds = {name: {"busy": 0.0, "waiting_in": 0.0, "waiting_out": 0.0} for name in ("source", "work", "sink")}

    # every method below that ends in _locked is called with self.cond held

    def fail(self, error):
        with self.cond:
            if self.error is None and not isinstance(error, _Stopped):
                self.error = error
            self.stopped = True
            self.cond.notify_all()

    def _finished_locked(self):
        return self.stopped or (self.source_done and self.sunk == self.produced)

    def _work_over_locked(self):
        return self.stopped or (self.source_done and self.sunk + len(self.results) == self.produced)

    def _spawn_locked(self, index):
        """A worker more for the replica when an item waits that no idle worker will take and the limit allows it."""
        rep = self.replicas[index]
        if len(rep.queue) > rep.idle and rep.workers < rep.limit and not self.stopped:
            rep.workers += 1
            t = threading.Thread(target=self._worker, args=(index,), name=f"pipeline-worker-{index}.{rep.made + rep.workers}", daemon=True)
            self.threads.append(t)
            t.start()

    # ---- source

    def _choose(self, state):
        if state["pending"] is None:
            t0 = time.perf_counter()
            with self.cond:
                while self.alive >= self.slots and not self.stopped:
                    self.cond.wait()
                state["waited"] += time.perf_counter() - t0
                if self.stopped:
                    raise _Stopped()
                n = len(self.replicas)
                order = [(self.last_choice + 1 + i) % n for i in range(n)]
                pick = min(order, key=lambda r: self.replicas[r].outstanding)     # (min keeps the first of equals: round-robin from the last one chosen)
                self.last_choice = pick
                self.replicas[pick].outstanding += 1
                self.alive += 1
                state["pending"] = pick
        return state["pending"]

    def _source(self):
        state = {"pending": None, "waited": 0.0}
        started = time.perf_counter()
        gen = None
        try:
            gen = self.source(lambda: self._choose(state))
            for item in gen:
                try:
                    pick = self._choose(state)
                except _Stopped:
                    self._release(item)
                    raise
                state["pending"] = None
                with self.cond:
                    if self.stopped:
                        self.replicas[pick].outstanding -= 1
                        self.alive -= 1
                        stopped = True
                    else:
                        stopped = False
                        self.replicas[pick].queue.append((self.produced, item))
                        self.produced += 1
                        self._spawn_locked(pick)
                        self.cond.notify_all()
                if stopped:
                    self._release(item)
                    raise _Stopped()
        except BaseException as e:   # noqa: B036 - kept for the caller
            self.fail(e)
        finally:
            if gen is not None and hasattr(gen, "close"):
                try:
                    gen.close()            # on this thread: what the generator holds open (a Prefetch) is shut here
                except BaseException as e:   # noqa: B036
                    self.fail(e)
            with self.cond:
                if state["pending"] is not None:      # chosen and never yielded: the end of the input
                    self.replicas[state["pending"]].outstanding -= 1
                    self.alive -= 1
                self.source_done = True
                self.cond.notify_all()
            total = time.perf_counter() - started
            self.seconds["source"]["waiting_out"] = state["waited"]
            self.seconds["source"]["busy"] = max(0.0, total - state["waited"])

    # ---- workers

    def _release(self, item):
        if self.release is not None:
            try:
                self.release(item)
            except BaseException as e:   # noqa: B036
                self.fail(e)

    def _worker(self, index):
        rep = self.replicas[index]
        obj, busy, waiting = None, 0.0, 0.0
        try:
            obj = self.factory(index)
            with self.cond:
                rep.made += 1
            while True:
                t0 = time.perf_counter()
                with self.cond:
                    rep.idle += 1
                    while not rep.queue and not self._work_over_locked():
                        self.cond.wait()
                    rep.idle -= 1
                    waiting += time.perf_counter() - t0
                    if self.stopped or not rep.queue:
                        return
                    seq, item = rep.queue.popleft()
                t0 = time.perf_counter()
                try:
                    result = self.work(obj, index, item)
                except RuntimeError as e:
                    busy += time.perf_counter() - t0
                    with self.cond:
                        retire = OUT_OF_MEMORY in str(e) and rep.limit > 1 and not self.stopped
                        if retire:     # this worker goes, its item goes back to the front for another one
                            rep.limit -= 1
                            rep.retired += 1
                            rep.workers -= 1
                            rep.queue.appendleft((seq, item))
                            self._spawn_locked(index)
                            self.cond.notify_all()
                    if retire:
                        rep = None     # (left the count already)
                        return
                    self._release(item)
                    raise
                except BaseException:
                    self._release(item)
                    raise
                busy += time.perf_counter() - t0
                with self.cond:
                    rep.outstanding -= 1
                    rep.items += 1
                    self.results[seq] = result
                    self.cond.notify_all()
                del result
                self._release(item)
        except BaseException as e:   # noqa: B036
            self.fail(e)
        finally:
            if obj is not None:
                try:
                    obj.close()
                except BaseException as e:   # noqa: B036
                    self.fail(e)
            with self.cond:
                if rep is not None:
                    rep.workers -= 1
                self.seconds["work"]["busy"] += busy
                self.seconds["work"]["waiting_in"] += waiting
                self.cond.notify_all()

    # ---- sink

    def _sink(self):
        busy = waiting = 0.0
        try:
            while True:
                t0 = time.perf_counter()
                with self.cond:
                    while self.sunk not in self.results and not self._finished_locked():
                        self.cond.wait()
                    waiting += time.perf_counter() - t0
                    if self.stopped or self.sunk not in self.results:
                        return
                    result = self.results.pop(self.sunk)
                t0 = time.perf_counter()
                self.sink(result)
                busy += time.perf_counter() - t0
                del result
                with self.cond:
                    self.sunk += 1
                    self.alive -= 1
                    self.cond.notify_all()
        except BaseException as e:   # noqa: B036
            self.fail(e)
        finally:
            self.seconds["sink"]["busy"], self.seconds["sink"]["waiting_in"] = busy, waiting

    # ---- the caller's thread

    def run(self):
        source = threading.Thread(target=self._source, name="pipeline-source", daemon=True)
        sink = threading.Thread(target=self._sink, name="pipeline-sink", daemon=True)
        try:
            source.start()
            sink.start()
            sink.join()
        except BaseException as e:   # noqa: B036 - an interrupt of the caller stops the stages too
            self.fail(e)
        finally:
            with self.cond:
                if not (self.source_done and self.sunk == self.produced):
                    self.stopped = True
                self.cond.notify_all()
            for t in (source, sink):
                if t.ident is not None:
                    t.join()
            joined = 0
            while True:                     # (a retiring worker may have started one more)
                with self.cond:
                    pending = self.threads[joined:]
                if not pending:
                    break
                for t in pending:
                    t.join()
                joined += len(pending)
            for rep in self.replicas:       # what a failed run never worked on
                for _, item in rep.queue:
                    self._release(item)
                rep.queue.clear()
            self.results.clear()
        if self.error is not None:
            raise self.error
        return {"items": self.sunk, "items_per_replica": [rep.items for rep in self.replicas], "workers_made": [rep.made for rep in self.replicas],
                "retired_workers": sum(rep.retired for rep in self.replicas), "limits": [rep.limit for rep in self.replicas],
                "stage_seconds": {name: {k: round(v, 6) for k, v in stage.items()} for name, stage in self.seconds.items()}}


def run(source, factory, work, sink, replicas=1, inflight=1, release=None):
    """Runs the pipeline to the end of the source (see the module's text). inflight: workers per replica, one number or one per replica.
    -> {"items", "items_per_replica", "workers_made", "retired_workers", "limits" (per replica, after retirements), "stage_seconds": {"source" | "work" | "sink":
    {"busy", "waiting_in", "waiting_out"}}} - "work" sums its worker threads; waiting_in is time spent waiting for the stage before, waiting_out for the one after."""
    return _Run(source, factory, work, sink, replicas, inflight, release).run()
