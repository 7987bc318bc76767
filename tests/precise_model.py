"""Precise clipping (--precise-clipping, preciseClipping / preciseClippingIdentityCutoff) and the X-drop (--X-drop, Xdropcutoff) of the reference's banded
extension, restated over tests/global_model.py:

- the error cost E = c / (1 - c) + 1 is a double (XscoreErrorCost, src/GraphAlignerCommon.h:108); the X score of a cell is (ScoreType)(cells - score * E): a double
  product, a double difference, truncated toward zero (WordSlice::getXScore, src/WordSlice.h:239-242);
- calculateNodeInner<PreciseClipping = true> (src/GraphAlignerBitvectorCommon.h:971-975,1148-1151) takes WordSlice::maxXScore of the node's entry column - before
  the merges of :977-1058 - and of every later column, and keeps the maximum. An early-leaving node returns the entry column's;
- calculateSlice (src/GraphAlignerBitvectorBanded.h:394-398) keeps the first strict maximum in node-pop order with its node, fillDPSlice (:456) adds slice.j; the
  initial slice has 0 at the seed's node (...Common.h:1259-1260); flattenLastSliceEnd is not called (:414);
- without an X-drop the slice loop is getViterbiSlices as BandModel / GlobalModel have it, and removeWronglyAlignedEnd is not called (:51,120);
- with one it is getXdropSlices (:703-830): every slice at the initial bandwidth, no stop, no ramp; bestXScore starts at the initial slice's 0; a slice whose score
  is below bestXScore - Xdropcutoff is dropped and ends the loop; scoresNotValid is set with >= (:768);
- the backtrace starts where getReverseTraceFromTableExactEndPos (...Common.h:321-383) puts it and walks by the unchanged rules.

With precise_clipping == 0 and x_drop == 0 the model is BandModel (force_global False) or GlobalModel (True), code path for code path. x_drop > 0 without a cut-off
runs with 0.66 (src/AlignerMain.cpp:443-448).

max_x_score_local_minima is WordSlice::maxXScoreLocalMinima (src/WordSlice.h:313-336) word for word on delta_words(col) - what the reference's release build runs;
max_x_score_cells is maxXScoreCellByCell (:264-272), which the reference only asserts against under EXTRACORRECTNESSASSERTIONS. The model decides by the former
and records every column it looked at in `columns_seen`, so that a test can hold the two against each other.

Rules fired: "clip: best slice is not the last", "clip: ends before the read's end", "clip: no exact end position" (the assertion at :377), "xdrop: stop",
"xdrop: first slice dropped"."""
import numpy as np

from band_model import BandModel
from extension_model import INT_MAX, W, Item, ModelAssertion, Slice, _check, _ComponentQueue, absent_previous, changed_min, column_step, delta_words, next_correctness, source_column
from global_model import GlobalModel

INT_MIN = -2 ** 31
_MASK = (1 << W) - 1


def error_cost(cutoff):
    return cutoff / (1.0 - cutoff) + 1.0


def x_score(cells, score, E):
    """(ScoreType)(cells - score * E): Python's float is the double, * and - round once each, int() truncates toward zero."""
    return int(cells - score * E)


def max_x_score_cells(col, E, cells=W):
    """maxXScoreCellByCell, src/WordSlice.h:264-272: row r holds r + 1 cells."""
    return max(x_score(r + 1, int(col[r + 1]), E) for r in range(min(W, cells)))


def max_x_score_words(vp, vn, score_before_start, E, cells=W):
    """maxXScoreLocalMinima, src/WordSlice.h:313-336, on the words."""
    priority_caused_minima = ~vp & _MASK
    possible = vp & ((priority_caused_minima - vp) & _MASK)
    possible >>= 1
    possible |= (1 << (W - 1)) & (priority_caused_minima | (~((priority_caused_minima - vp) & _MASK) & _MASK)) & (~vp & _MASK)
    result = INT_MIN
    possible |= 1
    while possible != 0:
        mask = possible ^ (possible - 1)
        cells_here = bin(mask).count("1")
        if cells_here > cells:
            break
        score_here = score_before_start + bin(vp & mask).count("1") - bin(vn & mask).count("1")
        result = max(result, x_score(cells_here, score_here, E))
        possible &= ~mask
    return result


def max_x_score_local_minima(col, E, cells=W):
    vp, vn = delta_words(col)
    return max_x_score_words(vp, vn, int(col[0]), E, cells)


class PreciseModel(GlobalModel):
    def __init__(self, graph, bandwidth, ramp_bandwidth=0, max_cells_per_slice=-1, force_global=False, precise_clipping=0.0, x_drop=0):
        super().__init__(graph, bandwidth, ramp_bandwidth, max_cells_per_slice)
        self.force_global = force_global
        self.x_drop = x_drop
        self.cutoff = precise_clipping if precise_clipping != 0 or x_drop <= 0 else 0.66
        self.clip = self.cutoff != 0
        self.E = error_cost(self.cutoff) if self.clip else None
        _check(not (x_drop > 0 and force_global), "getSlices: !forceGlobal")   # ...Banded.h:504
        self.columns_seen = []          # (VP, VN, scoreEnd) of every column whose maximum was taken
        self._node_max = None

    def _max_x(self, col, cells=W):
        vp, vn = delta_words(col)
        self.columns_seen.append((vp, vn, int(col[W])))
        return max_x_score_words(vp, vn, int(col[0]), self.E, cells)

    # -- calculateNodeInner<PreciseClipping = true>: the fold of the incoming columns (:903-964) once more, for the entry column's maximum (:973), then the node as it is
    def calculate_node(self, node, item, prev, incoming, sequence, j, prev_in_band, early_leave=True):
        if not self.clip or not early_leave:                                   # (early_leave False: recalcNodeWordslice, which takes no maximum)
            return super().calculate_node(node, item, prev, incoming, sequence, j, prev_in_band, early_leave)
        ws = None
        for (_, _, inc, skip_first) in incoming:
            if skip_first:
                ws = inc if ws is None else np.minimum(ws, inc)
                continue
            hin = (-1 if prev.start[W] < inc[0] else (1 if prev.start[W] > inc[0] else 0)) if prev.exists else 1
            new = column_step(inc, self._match(sequence, j, node, 0), hin)
            if not prev.exists or new[0] < prev.start[W]:
                new[0] = new[1] + 1
            ws = new if ws is None else np.minimum(ws, new)
        best = self._max_x(ws)
        result, ran_to_end = super().calculate_node(node, item, prev, incoming, sequence, j, prev_in_band, early_leave)
        if ran_to_end:
            for col in item.columns[1:]:
                best = max(best, self._max_x(col))
        self._node_max = best
        return result, ran_to_end

    # -- calculateSlice with PreciseClipping: BandModel's, with the maximum in pop order (:394-398) and without flattenLastSliceEnd (:414)
    def calculate_slice(self, sequence, j, cur, prev, prev_quit_score, bandwidth, prev_min_score):
        if not self.clip:
            return super().calculate_slice(sequence, j, cur, prev, prev_quit_score, bandwidth, prev_min_score)
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
        max_x, max_x_node = INT_MIN, None
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
            _check(self._node_max != INT_MIN, "nodeCalc.maxExactEndposScore set")                       # ...Banded.h:340
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
            if self._node_max > max_x:                                                                  # :394-398
                max_x, max_x_node = self._node_max, node
            _check(best[0] == slice_min, "result.minScore == currentMinScoreAtEndRow")
            cells += g.length[node] if ran_to_end else len(incoming)
            if self.max_cells is not None and cells > self.max_cells:
                if len(queue) > 0:
                    self._fire("cells: break")
                break
        _check(best[1] is not None, "minScoreNode set")
        cur.cells = cells
        self.slice_cells.append(cells)
        cur.max_x, cur.max_x_node = max_x + j, max_x_node                                               # fillDPSlice, :456-457
        return best

    def slices(self, sequence, bigraph_id, offset):
        if not self.clip:
            return GlobalModel.slices(self, sequence, bigraph_id, offset) if self.force_global else BandModel.slices(self, sequence, bigraph_id, offset)
        return self._xdrop_slices(sequence, bigraph_id, offset) if self.x_drop > 0 else self._viterbi_slices(sequence, bigraph_id, offset)

    def _initial(self, bigraph_id, offset):
        last = self.initial_slice(bigraph_id, offset)
        last.scores_not_valid = False
        last.max_x, last.max_x_node = 0, last.min_node                                                  # ...Common.h:1259-1260
        return last

    # -- getViterbiSlices (:513-701) as BandModel.slices / GlobalModel.slices state it; no removeWronglyAlignedEnd behind it (:51)
    def _viterbi_slices(self, sequence, bigraph_id, offset):
        num_slices = (len(sequence) + W - 1) // W
        last = self._initial(bigraph_id, offset)
        table = [last]
        _check(last.currently_correct(), "initial slice correct")
        ramp_on = self.ramp_bandwidth > self.bandwidth
        ramp_slice, ramp_redo, ramp_until = last, -1, 0
        s = 0
        while s < num_slices:
            bandwidth = self.ramp_bandwidth if ramp_on and ramp_until >= s else self.bandwidth
            new = Slice()
            new.j = last.j + W
            best = self.calculate_slice(sequence, new.j, new, last, last.min_score + last.bandwidth, bandwidth, last.min_score)
            new.min_score, new.min_node, new.min_offset = best
            _check(new.min_score >= last.min_score, "slice minimum never falls")
            next_correctness(last, new, new.min_score - last.min_score)
            new.bandwidth = bandwidth
            if ramp_until == s - 1 or (ramp_until < s and new.currently_correct() and new.false_from_correct):
                ramp_slice, ramp_redo = last, s - 1
            new.scores_not_valid = self.max_cells is not None and new.cells >= self.max_cells
            if not self.force_global:
                if not new.correct_from_correct:
                    self._fire("stop: not correct-from-correct")
                    break
                if not new.currently_correct() and ramp_until < s and ramp_on:
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
        return table

    # -- getXdropSlices, :703-830
    def _xdrop_slices(self, sequence, bigraph_id, offset):
        num_slices = (len(sequence) + W - 1) // W
        last = self._initial(bigraph_id, offset)
        table = [last]
        best_x = last.max_x
        for _ in range(num_slices):
            new = Slice()
            new.j = last.j + W
            best = self.calculate_slice(sequence, new.j, new, last, last.min_score + last.bandwidth, self.bandwidth, last.min_score)
            new.min_score, new.min_node, new.min_offset = best
            _check(new.min_score >= last.min_score, "slice minimum never falls")
            next_correctness(last, new, new.min_score - last.min_score)
            new.bandwidth = self.bandwidth
            if new.max_x > best_x:
                best_x = new.max_x
            new.scores_not_valid = self.max_cells is not None and new.cells >= self.max_cells           # :768
            if new.max_x < best_x - self.x_drop:
                self._fire("xdrop: stop" if len(table) > 1 else "xdrop: first slice dropped")
                break
            table.append(new)
            last = new
        return table

    # -- getReverseTraceFromTableExactEndPos, ...Common.h:321-383
    def exact_end(self, sequence, table):
        best_index = 1
        for i in range(1, len(table)):
            if table[i].max_x > table[best_index].max_x:
                best_index = i
        if best_index != len(table) - 1:
            self._fire("clip: best slice is not the last")
        sl, prev = table[best_index], table[best_index - 1]
        node, score = sl.max_x_node, sl.max_x
        _check(node in sl.items, "maxExactEndposNode in its slice")
        columns = self.tile_columns(node, sl.items[node], prev.items[node] if node in prev.items else absent_previous(), sequence, sl.j)
        cells = min(W, len(sequence) - sl.j)
        node_offset = bv_offset = None
        for i, col in enumerate(columns):
            max_score = max_x_score_local_minima(col, self.E, cells) + sl.j
            _check(max_score <= score, "maxScore <= score")                                             # :358
            if max_score == score:
                for off in range(W - 1, -1, -1):
                    if sl.j + off >= len(sequence):
                        continue
                    here = x_score(off + 1, int(col[off + 1]), self.E) + sl.j
                    _check(here <= score, "scoreHere <= score")                                         # :365
                    if here == score and (node_offset is None or off > bv_offset):
                        node_offset, bv_offset = i, off
        if node_offset is None:
            self._fire("clip: no exact end position")
            raise ModelAssertion("nodeOffset set")                                                      # :377
        if sl.j + bv_offset < len(sequence) - 1:
            self._fire("clip: ends before the read's end")
        return (node, node_offset, sl.j + bv_offset), int(columns[node_offset][bv_offset + 1])

    # -- getReverseTraceFromTable, ...Common.h:392-544, from a given cell: ExtensionModel.trace's walk
    def trace_from(self, sequence, table, pos):
        g = self.g
        trace = [pos]
        current = (None, None)
        columns = None
        while trace[-1][2] != -1:
            node, offset, seq_pos = trace[-1]
            si = seq_pos // W + 1
            _check(si < len(table), "trace inside the table")
            cur, prev = table[si], table[si - 1]
            if current != (si, node):
                current = (si, node)
                _check(node in cur.items, "trace node in slice")
                columns = self.tile_columns(node, cur.items[node], prev.items[node] if node in prev.items else absent_previous(), sequence, cur.j)
            _check(offset < g.length[node], "offset inside node")
            if seq_pos % W == 0 and offset == 0:
                trace.append(self._corner(cur, prev, node, sequence))
                self._no_cycle(trace)
                continue
            if seq_pos % W == 0:
                if node not in prev.items:
                    self._fire("trace: first row of a node new in this slice")
                    trace.append((node, 0, seq_pos))
                    continue
                first, second = self._vertical_crossing(cur, prev, columns, node, trace[-1], sequence)
                if first[1] != trace[-1][1]:
                    for off in range(trace[-1][1] - 1, first[1], -1):
                        trace.append((first[0], off, first[2]))
                if first != trace[-1]:
                    trace.append(first)
                _check(second != trace[-1], "crossing moves")
                trace.append(second)
                continue
            if offset == 0:
                first, second = self._horizontal_crossing(cur, prev, node, trace[-1], sequence)
                if first[2] != trace[-1][2]:
                    for sp in range(trace[-1][2] - 1, first[2], -1):
                        trace.append((first[0], first[1], sp))
                if first != trace[-1]:
                    trace.append(first)
                _check(second != trace[-1], "crossing moves")
                trace.append(second)
                self._no_cycle(trace)
                continue
            trace.extend(self._inside(cur.j, columns, trace[-1], sequence))
        node = trace[-1][0]
        _check(node in table[0].items, "trace ends on an initial node")
        it = table[0].items[node]
        before = [int(it.start[W])]
        for i in range(1, g.length[node]):
            before.append(before[-1] + it.bottom[i])
        _check(before[-1] == int(it.end[W]), "ramp ends at endSlice")
        while before[trace[-1][1]] != 0 and trace[-1][1] > 0 and before[trace[-1][1] - 1] == before[trace[-1][1]] - 1:
            trace.append((node, trace[-1][1] - 1, trace[-1][2]))
        if trace[-1][1] == 0 and before[0] != 0:
            for nb in g.inn[node]:
                if nb in table[0].items and int(table[0].items[nb].end[0]) == before[0] - 1:
                    self._fire("trace: step into an in-neighbour above the first slice")
                    trace.append((nb, g.length[nb] - 1, trace[-1][2]))
                    break
        return trace

    # -- getReverseTraceFromSeed, ...Banded.h:46-71
    def extend(self, sequence, bigraph_id, offset):
        if not self.clip:
            return super().extend(sequence, bigraph_id, offset)
        self._eq = {}
        table = self.slices(sequence, bigraph_id, offset)
        out = {
            "slice_min": [s.min_score for s in table],
            "slice_max_x": [(s.max_x, s.max_x_node) for s in table],
            "slice_nodes": [sorted(s.items) for s in table],
            "failed": len(table) <= 1, "score": None, "trace": [],
        }
        if len(table) > 1:
            _check(0 <= table[-1].min_score <= len(sequence) + 2 * W, "last slice's minimum in range")  # :57-58
            pos, out["score"] = self.exact_end(sequence, table)
            out["trace"] = self.trace_from(sequence, table, pos)
        return out
