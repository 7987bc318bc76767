"""The band controls of the reference's banded extension, restated over tests/extension_model.py's cell-matrix model:

- the ramp (--ramp-bandwidth, rampBandwidth): getViterbiSlices, src/GraphAlignerBitvectorBanded.h:530-644;
- the cell limit per slice (--tangle-effort, maxCellsPerSlice): calculateSlice's break, :400-405, the scoresNotValid flag, :579-584, and the
  backtrace rules that read it, src/GraphAlignerBitvectorCommon.h:599-804.

ExtensionModel is the reference with both off; BandModel(graph, bandwidth) with the defaults (ramp 0, no limit) runs exactly its code paths.
The rules fire "ramp: rewind", "cells: break" and "cells: scores not valid" (a backtrace choice that the flag changed) when they apply."""
import numpy as np

from extension_model import (INT_MAX, W, ExtensionModel, Item, ModelAssertion, Slice, _check, _ComponentQueue, absent_previous, changed_min,
                             next_correctness, source_column)


class _NotValid:
    """A slice whose scores are not valid, as the backtrace rules see it: every "score > quitScore" test holds (the reference tests
    `scoresNotValid || score > quitScore`, ...Common.h:614,690,713,776), so its bandwidth is taken as minus infinity there."""

    def __init__(self, s):
        self._s = s

    def __getattr__(self, name):
        if name == "bandwidth":
            return -(1 << 62)
        return getattr(self._s, name)


class BandModel(ExtensionModel):
    def __init__(self, graph, bandwidth, ramp_bandwidth=0, max_cells_per_slice=-1):
        super().__init__(graph, bandwidth)
        self.ramp_bandwidth = ramp_bandwidth
        self.max_cells = None if max_cells_per_slice < 0 else max_cells_per_slice
        self.slice_cells = []                  # cellsProcessed of every slice computed (redone ones included), for tests that pick a limit
        self._plain = False                    # (inside _with_flags: the rules run as if no flag were set)

    # -- calculateSlice, ...Banded.h:205-426, with the cell count: a node counts what calculateNodeInner leaves in cellsProcessed - its columns
    #    when it runs to its end (:1162), its incoming entries when it leaves early (:903-905, :989-1046)
    def calculate_slice(self, sequence, j, cur, prev, prev_quit_score, bandwidth, prev_min_score):
        g = self.g
        queue = _ComponentQueue()
        for node, it in prev.items.items():
            if j == 0:
                _check(it.min_score <= prev_quit_score, "initial node inside the band")
            else:
                _check(it.exists, "previous item exists")
                if it.min_score > prev_quit_score:
                    self._fire("start: node outside the previous band")
                    continue
                if g.linearizable[node]:
                    nb = g.inn[node][0]
                    if nb in prev.items and prev.items[nb].end[W] < prev_quit_score and prev.items[nb].min_score < prev_quit_score:
                        self._fire("start: left to its only predecessor")
                        continue
            queue.insert(g.component[node], it.min_score, (node, it.min_score - prev_min_score, source_column(int(it.start[W])), True))
        _check(len(queue) > 0, "queue not empty")
        slice_min = INT_MAX - bandwidth - 1
        best = (slice_min, None, None)
        cells = 0
        while len(queue) > 0:
            node = queue.top()
            if not queue.extras.get(node):
                queue.pop()
                continue
            if node not in cur.items:
                cur.items[node] = Item()
            item = cur.items[node]
            old_end = item.end.copy() if item.exists else np.full(W + 1, INT_MAX, dtype=np.int64)
            prev_item = prev.items[node].copy() if node in prev.items else absent_previous()
            incoming = list(queue.extras[node])
            calc, ran_to_end = self.calculate_node(node, item, prev_item, incoming, sequence, j, lambda v: v in prev.items)
            queue.pop()
            _check(calc[0] <= prev_quit_score + bandwidth + W + W, "node minimum inside the reachable range")
            slice_min = min(slice_min, calc[0])
            item.min_score = min(item.min_score, calc[0])
            new_end = item.end
            if not np.array_equal(new_end, old_end):
                end_min = changed_min(new_end, old_end)
                _check(end_min >= prev_min_score and end_min != INT_MAX, "changed minimum")
                if end_min > slice_min + bandwidth:
                    self._fire("band rule: change not passed on")
                if end_min <= slice_min + bandwidth:
                    for nb in g.out[node]:
                        queue.insert(g.component[nb], end_min, (nb, end_min - prev_min_score, new_end, False))
            if calc[0] < best[0]:
                best = (calc[0], node, calc[1])
            _check(best[0] == slice_min, "result.minScore == currentMinScoreAtEndRow")
            cells += g.length[node] if ran_to_end else len(incoming)
            if self.max_cells is not None and cells > self.max_cells:       # :405: the rest of the queue is dropped
                if len(queue) > 0:
                    self._fire("cells: break")
                break
        _check(best[1] is not None, "minScoreNode set")
        cur.cells = cells
        self.slice_cells.append(cells)
        if j + W > len(sequence):
            best = self.flatten_last_slice(cur, prev, sequence, j)
        return best

    # -- getViterbiSlices, ...Banded.h:513-701 with the ramp, + removeWronglyAlignedEnd, ...Common.h:1231-1241
    def slices(self, sequence, bigraph_id, offset):
        num_slices = (len(sequence) + W - 1) // W
        last = self.initial_slice(bigraph_id, offset)
        last.scores_not_valid = False
        table = [last]
        _check(last.currently_correct(), "initial slice correct")
        ramp_on = self.ramp_bandwidth > self.bandwidth
        ramp_slice, ramp_redo, ramp_until = last, -1, 0
        s = 0
        while s < num_slices:
            bandwidth = self.ramp_bandwidth if ramp_on and ramp_until >= s else self.bandwidth   # :544 (slice 0 always: rampUntil starts at 0)
            new = Slice()
            new.j = last.j + W
            best = self.calculate_slice(sequence, new.j, new, last, last.min_score + last.bandwidth, bandwidth, last.min_score)
            new.min_score, new.min_node, new.min_offset = best
            _check(new.min_score >= last.min_score, "slice minimum never falls")
            next_correctness(last, new, new.min_score - last.min_score)
            new.bandwidth = bandwidth
            if ramp_until == s - 1 or (ramp_until < s and new.currently_correct() and new.false_from_correct):   # :572-576 (s - 1 wraps at s = 0 there: never equal)
                ramp_slice, ramp_redo = last, s - 1
            new.scores_not_valid = self.max_cells is not None and new.cells >= self.max_cells          # :581-584 (>=, where the break has >)
            if not new.correct_from_correct:
                self._fire("stop: not correct-from-correct")
                break
            if not new.currently_correct() and ramp_until < s and ramp_on:                                 # :608-644
                self._fire("ramp: rewind")
                ramp_until = s
                s, ramp_redo = ramp_redo, s
                last, ramp_slice = ramp_slice, last
                if s == -1:
                    table = []
                while len(table) > 1 and table[-1].j > s * W:
                    table.pop()
                _check(s == -1 or len(table) == s + 2, "kept slices end at the redo point")
                _check(table[-1].j == last.j, "redo starts behind the snapshot")
                s += 1
                continue
            table.append(new)
            last = new
            s += 1
        currently_correct = table[-1].currently_correct()
        while not currently_correct:
            self._fire("trim: slice dropped")
            currently_correct = table[-1].false_from_correct
            table.pop()
            if not table:
                break
        return table

    # -- the backtrace's crossing and corner rules with scoresNotValid (...Common.h:599-804): a slice flagged not valid takes the "outside the band" branch
    def _band_view(self, cur, prev):
        if self._plain:
            return cur, prev
        c = _NotValid(cur) if getattr(cur, "scores_not_valid", False) else cur
        p = _NotValid(prev) if getattr(prev, "scores_not_valid", False) else prev
        return c, p

    def _with_flags(self, plain, flagged):
        """Runs a rule with the flags; when a flag is set, also without them, to tell whether the flag decided the choice."""
        got = flagged()
        self._plain = True
        try:
            unflagged = plain()
        except ModelAssertion:
            unflagged = None
        finally:
            self._plain = False
        if got != unflagged:
            self._fire("cells: scores not valid")
        return got

    def _horizontal_crossing(self, cur, prev, node, pos, sequence):
        c, p = self._band_view(cur, prev)
        if c is cur and p is prev:
            return super()._horizontal_crossing(cur, prev, node, pos, sequence)
        base = super()._horizontal_crossing
        return self._with_flags(lambda: base(cur, prev, node, pos, sequence), lambda: base(c, p, node, pos, sequence))

    def _vertical_crossing(self, cur, prev, columns, node, pos, sequence):
        c, p = self._band_view(cur, prev)
        if c is cur and p is prev:
            return super()._vertical_crossing(cur, prev, columns, node, pos, sequence)
        base = super()._vertical_crossing
        return self._with_flags(lambda: base(cur, prev, columns, node, pos, sequence), lambda: base(c, p, columns, node, pos, sequence))

    def _corner(self, cur, prev, node, sequence):
        if isinstance(cur, _NotValid) or isinstance(prev, _NotValid):       # (called from a crossing that already holds the flagged views)
            return super()._corner(cur, prev, node, sequence)
        c, p = self._band_view(cur, prev)
        if c is cur and p is prev:
            return super()._corner(cur, prev, node, sequence)
        base = super()._corner
        return self._with_flags(lambda: base(cur, prev, node, sequence), lambda: base(c, p, node, sequence))

