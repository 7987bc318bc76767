"""The forced global alignment (--global-alignment, forceGlobal: src/AlignerMain.cpp:66,160,299) of the reference's banded extension, restated over
tests/band_model.py:

- getViterbiSlices, src/GraphAlignerBitvectorBanded.h:513-701, skips its whole `if (!forceGlobal)` block (:587-645): a slice that is not
  correct-from-correct is kept, and the ramp never rewinds. rampUntil therefore stays 0, and the band choice of :544 gives the ramp bandwidth to
  slice 0 and to no other slice. The cell limit's break and its scoresNotValid flag (:400-405, :579-584) are as in BandModel.
- getBacktraceFullStart / getSlicesAndTrace (:46-71, :120) do not call removeWronglyAlignedEnd.

The correctness state is still advanced every slice; nothing reads it. The rules fire "global: kept past not correct-from-correct" when a slice is
kept at which the default would have stopped, and "global: wrong end kept" when the last slice is not currently correct."""
from band_model import BandModel
from extension_model import W, Slice, _check, next_correctness


class GlobalModel(BandModel):
    def slices(self, sequence, bigraph_id, offset):
        num_slices = (len(sequence) + W - 1) // W
        last = self.initial_slice(bigraph_id, offset)
        last.scores_not_valid = False
        table = [last]
        _check(last.currently_correct(), "initial slice correct")
        ramp_on = self.ramp_bandwidth > self.bandwidth
        for s in range(num_slices):
            bandwidth = self.ramp_bandwidth if ramp_on and s == 0 else self.bandwidth   # :544 with rampUntil == 0 throughout
            new = Slice()
            new.j = last.j + W
            best = self.calculate_slice(sequence, new.j, new, last, last.min_score + last.bandwidth, bandwidth, last.min_score)
            new.min_score, new.min_node, new.min_offset = best
            _check(new.min_score >= last.min_score, "slice minimum never falls")
            next_correctness(last, new, new.min_score - last.min_score)
            new.bandwidth = bandwidth
            new.scores_not_valid = self.max_cells is not None and new.cells >= self.max_cells   # :581-584
            if not new.correct_from_correct:
                self._fire("global: kept past not correct-from-correct")
            table.append(new)
            last = new
        if not table[-1].currently_correct():
            self._fire("global: wrong end kept")
        return table
