"""The tool as plain GraphAligner (--no-colinear-chaining) with the seed-extension heuristics, read a second time from the reference's sources in plain Python;
nothing is imported from oracle/ or the product.

  GraphAlignerModel.align_one_way   AlignOneWay, src/GraphAligner.h:114-203, with seedExtendDensity (--seeds-extend-density) and nondeterministicOptimizations
                                    (--extra-heuristic) as parameters: the three rules at :127, :132 and :152 in the reference's order
  EValue                            EValueCalculator, src/EValue.cpp:16-113 (the 70 % identity model of src/Aligner.cpp:478-482)
  alignment_incompatible            src/AlignmentSelection.cpp:9-31 (the cut-off is a C float)
  select_alignments                 SelectAlignments, src/AlignmentSelection.cpp:53-99, GreedySelectAlignments and ScheduleSelectAlignments, src/AlignmentSelection.h:36-96

select_alignments takes and returns (start, end, score) triples by INDEX into the list it was given, in the order the reference returns the alignments. Its sorts go through
`std_sort` (the local libstdc++'s std::sort as a permutation function, tests/stdsort/std_sort_perm.cpp): a comparator over exact keys is a sort of the keys' ranks."""
import functools
import math
import struct

from alignment_model import AlignmentModel, reverse_complement

GREEDY_LENGTH, GREEDY_SCORE, GREEDY_E, SCHEDULE_INVERSE_E_SUM, SCHEDULE_INVERSE_E_PRODUCT, SCHEDULE_SCORE, SCHEDULE_LENGTH, ALL = range(8)   # SelectionMethod, src/AlignmentSelection.h:14-24


def extend_seeds_budget(density, read_length, n_seeds):
    """size_t extendSeeds = seedExtendDensity * sequence.size() + 1 (a double, truncated); -1: every seed (src/GraphAligner.h:121-122)."""
    return n_seeds if density == -1 else int(density * read_length + 1)


class GraphAlignerModel(AlignmentModel):
    def align_one_way(self, sequence, seeds, sloppy, min_cluster_size=1, l=0, r=None, offset=0, seed_extend_density=-1, extra_heuristic=False):
        """As AlignmentModel.align_one_way, with the two controls the chaining presets fix. Returns (alignments in the list's final order, seeds extended)."""
        r = len(seeds) if r is None else r
        rev_sequence = reverse_complement(sequence)
        alignments, extended = [], 0
        end_to_end_score = 0
        extend_seeds = extend_seeds_budget(seed_extend_density, len(sequence), len(seeds))
        worst_extended = 0
        for i in range(l, min(len(seeds), r)):
            goodness = seeds[i]["goodness"]
            if sloppy and ((extra_heuristic and goodness == end_to_end_score) or goodness < end_to_end_score):          # :127
                break
            if extended >= extend_seeds and (extra_heuristic or goodness < worst_extended):                              # :132
                break
            seed = dict(seeds[i])
            seed["seqPos"] -= offset
            if seed["cluster"] < min_cluster_size:                                                                      # :141
                continue
            if sloppy and any(a["start"] <= seed["seqPos"] <= a["end"] and (extra_heuristic or a["goodness"] > seed["goodness"]) for a in alignments):   # :152
                continue
            if any(self.exact_alignment_part(a, seed) for a in alignments):                                             # :163-173
                continue
            worst_extended = seed["goodness"]                                                                           # :175-176: a failed extension counts
            extended += 1
            item = self.alignment_from_seed(sequence, rev_sequence, seed)
            if item is None:
                continue
            item["goodness"] = seed["goodness"]
            alignments.append(item)
            if sloppy:
                alignments.sort(key=lambda a: a["start"])       # (std::sort by alignmentStart: what follows reads the list in that order, ties do not change its outcome)
                if alignments[0]["start"] == 0:
                    min_goodness, contiguous_end = alignments[0]["goodness"], alignments[0]["end"]
                    for a in alignments[1:]:
                        if a["start"] <= contiguous_end:
                            min_goodness = min(min_goodness, a["goodness"])
                            contiguous_end = max(contiguous_end, a["end"])
                    if contiguous_end == len(sequence):
                        end_to_end_score = min_goodness
        return alignments, extended


_E = 2.71828182845904523536028747135266249775724709369995


class EValue:
    def __init__(self, min_identity=0.7):
        self.match, self.mismatch = 1.0, -min_identity / (1.0 - min_identity)
        lo, hi = 0.0, 0.7                                      # initializeLambda: bisection, at most 100 steps
        for _ in range(100):
            mid = (lo + hi) * 0.5
            value = math.pow(_E, mid * self.match) * .5 + math.pow(_E, mid * self.mismatch) * 0.5 - 1
            if value < 0:
                lo = mid
            if value > 0:
                hi = mid
            if value == 0:
                lo = hi = mid
                break
            if lo == hi:
                break
        self.lam = (lo + hi) / 2
        series, triangle = 0.0, [1]                            # initializeK
        for k in range(1, 10):
            new = [0] * (len(triangle) + 1)
            for j, v in enumerate(triangle):
                new[j] += v
                new[j + 1] += v
            triangle = new
            total = sum(triangle)
            negative = greater = 0.0
            for j, v in enumerate(triangle):
                score = float(j) * self.match + float(len(triangle) - 1 - j) * self.mismatch
                p = float(v) / float(total)
                if score < 0:
                    negative += math.pow(_E, self.lam * score) * p
                if score >= 0:
                    greater += p
            series += (negative + greater) / float(k)
        expectation = .5 * self.match * math.pow(_E, self.lam * self.match) + .5 * self.mismatch * math.pow(_E, self.lam * self.mismatch)
        c_star = math.pow(_E, -2 * series) / (self.lam * expectation)
        self.K = c_star * self.lam / (1.0 - math.pow(_E, -self.lam))

    def alignment_score(self, length, edits):
        return length * self.match - edits * (self.mismatch - self.match)

    def evalue(self, m, n, length, edits):
        try:
            return self.K * m * n * math.pow(_E, -self.lam * self.alignment_score(length, edits))
        except OverflowError:                                   # (C's pow returns +inf where Python raises)
            return math.inf


def _c_float(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def alignment_incompatible(left, right):
    """An overlap larger than 5 % of the shorter alignment; the product size_t * float is a float, and the int overlap is compared with it as a float."""
    min_overlap = _c_float(_c_float(float(min(left[1] - left[0], right[1] - right[0]))) * _c_float(0.05))
    (ls, le), (rs, re_) = left[:2], right[:2]
    if ls > rs:
        ls, le, rs, re_ = rs, re_, ls, le
    overlap = le - rs if le > rs else 0
    return _c_float(float(overlap)) > min_overlap


def _sort_indices(n, less, std_sort):
    """std::sort of 0..n-1 with the strict weak order `less`: the elements' ranks in that order are integer keys with the same comparison outcomes."""
    by_rank = sorted(range(n), key=functools.cmp_to_key(lambda a, b: -1 if less(a, b) else (1 if less(b, a) else 0)))
    rank, at = [0] * n, 0
    for k, i in enumerate(by_rank):
        if k and less(by_rank[k - 1], i):
            at += 1
        rank[i] = at
    return list(std_sort(rank)) if n else []


def _greedy(alns, less, std_sort):
    result = []
    for i in _sort_indices(len(alns), lambda a, b: less(alns[a], alns[b]), std_sort):
        if not any(alignment_incompatible(alns[e], alns[i]) for e in result):
            result.append(i)
    return result


def _schedule(alns, scorer, std_sort):
    if not alns:                                                # (the reference reads items[0] of an empty list here; an empty selection stands in for that)
        return []
    items = _sort_indices(len(alns), lambda a, b: alns[a][1] < alns[b][1], std_sort)
    backtrace, score = [None] * len(items), [0.0] * len(items)
    for i in range(len(items)):
        raw = scorer(alns[items[i]])
        score[i] = raw
        for j in range(i):
            if alignment_incompatible(alns[items[i]], alns[items[j]]):
                continue
            if score[j] + raw > score[i]:
                backtrace[i], score[i] = j, score[j] + raw
    at = 0
    for i in range(len(items)):
        if score[i] > score[at]:
            at = i
    result = []
    while at is not None:
        result.append(items[at])
        at = backtrace[at]
    return result


def _div(a, b):                                                # IEEE division, as C++ doubles divide
    if b == 0:
        return math.nan if a == 0 or a != a else math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def _neg_log(x):
    if x == 0:
        return math.inf
    return -math.log(x) if x != math.inf else -math.inf


def select_alignments(alns, method, graph_size, read_size, e_cutoff, std_sort, evalue=None):
    """alns: [(start, end, score)]. Returns the indices SelectAlignments keeps, in the order it returns them: --E-cutoff first, then `method`."""
    ev = evalue or _default_evalue()
    kept = [i for i, a in enumerate(alns) if e_cutoff == -1 or ev.evalue(graph_size, read_size, a[1] - a[0], a[2]) <= e_cutoff]
    sub = [alns[i] for i in kept]

    def e_of(a):
        return ev.evalue(graph_size, read_size, a[1] - a[0], a[2])

    def score_of(a):
        return ev.alignment_score(a[1] - a[0], a[2])
    if method == GREEDY_LENGTH:
        picked = _greedy(sub, lambda l, r: (l[1] - l[0]) > (r[1] - r[0]) or ((l[1] - l[0]) == (r[1] - r[0]) and l[2] < r[2]), std_sort)
    elif method == GREEDY_SCORE:
        picked = _greedy(sub, lambda l, r: score_of(l) > score_of(r), std_sort)
    elif method == GREEDY_E:
        picked = _greedy(sub, lambda l, r: e_of(l) < e_of(r), std_sort)
    elif method == SCHEDULE_INVERSE_E_SUM:
        picked = _schedule(sub, lambda a: _div(1.0, e_of(a)), std_sort)
    elif method == SCHEDULE_INVERSE_E_PRODUCT:
        picked = _schedule(sub, lambda a: _neg_log(e_of(a)), std_sort)
    elif method == SCHEDULE_SCORE:
        picked = _schedule(sub, score_of, std_sort)
    elif method == SCHEDULE_LENGTH:
        picked = _schedule(sub, lambda a: (a[1] - a[0]) + 0.5 - _div(0.5, float(a[2])), std_sort)
    else:
        picked = list(range(len(sub)))
    return [kept[i] for i in picked]


@functools.lru_cache(maxsize=None)
def _default_evalue():
    return EValue(0.7)
