"""tests/corrected_model.py on hand cases: each expected string is worked out by hand from the reference's three functions (src/GraphAligner.h:220-231,
src/ReadCorrection.cpp:22-64, src/Aligner.cpp:313-374). The order of a read's alignments (output_order: std::sort by start, twice) is worked out from the permutation
function of tests/stdsort, on a hand case and on the tandem-array reads that tests/test_corrected_modes_gpu.py runs on the device."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np                          # noqa: E402

import corrected_model as cm                # noqa: E402
from test_seeding_model import std_sort     # noqa: E402,F401  (the fixture: libstdc++'s std::sort as a permutation function)

# two nodes: 0 = "ACGTRN" (an IUPAC code and an N in the graph), 2 = "TTGCA"
NODES = {0: b"ACGTRN", 2: b"TTGCA"}


def letter(node, offset):
    return NODES[node][offset:offset + 1]


def walk(node, a, b, switch_last=False):
    cells = [(node, o, 0) for o in range(a, b)]
    if switch_last:
        cells[-1] = (node, b - 1, 1)
    return cells


def test_matches_only_spell_the_path():
    assert cm.add_corrected(walk(0, 0, 6), letter) == b"ACGTRN"
    assert cm.add_corrected([(0, 3, 0)], letter) == b"T"
    assert cm.add_corrected(walk(0, 4, 6, switch_last=True) + walk(2, 0, 3), letter) == b"RNTTG"


def test_an_insertion_run_adds_nothing():
    # read bases against one graph position: the position repeats without a node switch
    trace = [(0, 0, 0), (0, 1, 0), (0, 1, 0), (0, 1, 0), (0, 1, 0), (0, 2, 0)]
    assert cm.add_corrected(trace, letter) == b"ACG"
    # an insertion at the very start: cell 0 is always taken, its repeats are not
    assert cm.add_corrected([(2, 4, 0), (2, 4, 0), (2, 4, 0)], letter) == b"A"


def test_a_deletion_run_adds_its_letters():
    # a deletion advances in the graph with the read position unchanged: the rule never looks at the read position
    trace = [(0, 0, 0), (0, 1, 0), (0, 2, 0), (0, 3, 0), (0, 4, 0)]
    assert cm.add_corrected(trace, letter) == b"ACGTR"


def test_a_repeated_position_behind_a_node_switch_is_kept():
    # only a cycle could reach it; the rule is written with !nodeSwitch first
    trace = [(2, 4, 1), (2, 4, 0), (2, 4, 0)]
    assert cm.add_corrected(trace, letter) == b"AA"
    # the same offset in another node is another position
    assert cm.add_corrected([(0, 2, 0), (2, 2, 0)], letter) == b"GG"


RAW = b"acgtNNRYacgtACGTacgt"   # 20 letters: lower case and IUPAC codes in the read


def test_gap_abutting_and_tail():
    got = cm.get_corrected(RAW, [(2, 6, b"ggtt"), (6, 10, b"AaCc"), (14, 16, b"TT")])
    #        raw[0:2] lower | piece | abutting piece, upper-cased | raw[10:14] lower | piece | tail raw[16:] lower
    assert got == b"ac" + b"GGTT" + b"AACC" + b"gtac" + b"TT" + b"acgt"


def test_an_overlapping_piece_is_appended_whole_when_max_overlap_is_zero():
    got = cm.get_corrected(RAW, [(0, 8, b"ACGTACGT"), (5, 12, b"CGTAAAA")])
    assert got == b"ACGTACGT" + b"CGTAAAA" + b"acgtacgt"       # nothing trimmed: getLongestOverlap(.., 0) is 0; the tail starts at 12


def test_an_end_that_moves_current_end_backwards():
    # the second alignment starts inside the first and ends before it did: currentEnd goes from 12 back to 9, the third starts at 10 > 9 and raw[9:10] is written again
    got = cm.get_corrected(RAW, [(0, 12, b"A" * 12), (4, 9, b"CCCCC"), (10, 20, b"G" * 10)])
    assert got == b"A" * 12 + b"CCCCC" + RAW[9:10].lower() + b"G" * 10


def test_no_alignment_gives_the_lower_cased_read():
    assert cm.get_corrected(RAW, []) == b"acgtnnryacgtacgtacgt"
    assert cm.corrected_record(b"read one extra words", RAW, []) == b">read one extra words\nacgtnnryacgtacgtacgt\n"


def test_lower_case_and_codes_in_the_read_and_the_piece():
    # tolower of the raw stretches keeps the codes as letters; toupper of a piece that holds codes keeps them
    got = cm.get_corrected(b"ACNRYKacgu", [(3, 5, b"rn")])
    assert got == b"acn" + b"RN" + b"kacgu"


def test_get_longest_overlap_indexes_from_max_overlap():
    # left ends in ...GATTA; the window always starts maxOverlap letters before left's end, whatever length i is tried
    assert cm.get_longest_overlap(b"CCGATTA", b"GATTACA", 5) == 5
    # "TTA" is a suffix of left and a prefix of right, but the window starts 5 back (at 'G'), so no i < 5 can match: 0, not 3
    assert cm.get_longest_overlap(b"CCGATTA", b"TTAGG", 5) == 0
    # maxOverlap is cut to the shorter side first
    assert cm.get_longest_overlap(b"TA", b"TACC", 5) == 2
    assert cm.get_longest_overlap(b"TA", b"T", 5) == 0          # window starts 1 back: left[1] = 'A' != 'T'
    # i < maxOverlap matches when the window's first i letters are right's prefix
    assert cm.get_longest_overlap(b"CCGATTA", b"GAC", 5) == 0    # cut to 3: window "TTA"
    assert cm.get_longest_overlap(b"AAGAT", b"GAC", 3) == 2      # window "GAT": "GAC"[:2] == "GA"
    assert cm.get_corrected(RAW, [(0, 8, b"ACGTACGT"), (5, 12, b"CGTAAAA")], max_overlap=3) == b"ACGTACGT" + b"AAAA" + b"acgtacgt"


def test_record_formats():
    corrections = [(2, 6, b"ggtt"), (14, 16, b"TN")]
    assert cm.corrected_record(b"r1 desc", RAW, corrections) == b">r1 desc\nacGGTTryacgtacTNacgt\n"
    assert cm.clipped_records(b"r1 desc", corrections) == [b">r1 desc_0_2_6\nggtt\n", b">r1 desc_1_14_16\nTN\n"]
    assert cm.clipped_records(b"r1", []) == []


# ---- the order of a read's alignments: src/Aligner.cpp:1003 and :1023 sort by alignmentStart with libstdc++'s std::sort, twice


def _stable(keys):
    return sorted(range(len(keys)), key=lambda i: keys[i])


def tied_keys(std_sort, n=24, distinct=5):   # noqa: F811
    """`n` > 16 keys over `distinct` values on which two std::sorts, one std::sort and a stable sort give three different orders: the first such list of a
    fixed-seed search, found with the permutation function itself."""
    import random
    rng = random.Random(5)
    for _ in range(2000):
        keys = [rng.randrange(distinct) for _ in range(n)]
        once, twice, stable = cm.output_order(keys, std_sort, sorts=1), cm.output_order(keys, std_sort), _stable(keys)
        if len({tuple(once), tuple(twice), tuple(stable)}) == 3:
            return keys, once, twice, stable
    raise AssertionError("no list of tied keys tells the three orders apart")


def test_the_output_order_is_the_sort_replayed_twice(std_sort):   # noqa: F811
    keys, once, twice, stable = tied_keys(std_sort)
    print("keys", keys, "once", once, "twice", twice, "stable", stable)
    assert len(keys) >= 17 and len(set(keys)) < len(keys)
    for order in (once, twice, stable):                                        # three orders of the same keys, each sorted, no two alike
        assert sorted(order) == list(range(len(keys))) and [keys[i] for i in order] == sorted(keys)
    assert once != twice and twice != stable and once != stable
    assert twice == [once[i] for i in std_sort([keys[i] for i in once])]       # the second sort works on what the first one left
    assert cm.output_order(keys) == stable                                     # without the function: the stable order, as before
    # up to 16 elements std::sort is an insertion sort: stable, once or twice
    assert all(cm.output_order(keys[:n], std_sort) == cm.output_order(keys[:n], std_sort, sorts=1) == _stable(keys[:n]) for n in range(17))
    # through result_corrections: one read, every alignment one cell long, its letter naming the alignment
    n = len(keys)
    out = {"failed_assertion": [0], "capacity_exceeded": [0], "chained_better": [0], "read_longall_off": [0, n], "read_long_off": [0, n], "long_index": list(range(n)),
           "longall_start": keys, "longall_end": [k + 1 for k in keys], "long_trace_off": list(range(n + 1)),
           "long_trace_node": np.arange(n), "long_trace_offset": np.zeros(n, dtype=np.int64), "long_trace_switch": np.zeros(n, dtype=np.int64)}
    name = lambda node, offset: b"%c" % (65 + node)                            # noqa: E731
    assert [c[2] for c in cm.result_corrections(out, 0, name, std_sort)] == [b"%c" % (65 + i) for i in twice]
    assert [c[2] for c in cm.result_corrections(out, 0, name)] == [b"%c" % (65 + i) for i in stable]
    out["long_index"] = list(range(n))[::-1]                                   # the sort starts from the selection's order, not from the list's
    reverse = [n - 1 - i for i in cm.output_order(keys[::-1], std_sort)]
    assert [c[2] for c in cm.result_corrections(out, 0, name, std_sort)] == [b"%c" % (65 + i) for i in reverse]
    bodies, clipped = cm.batch_records(out, [b"r"], [b"a" * 8], name, std_sort)
    assert len(bodies) == 1 and [c.split(b"\n")[1] for c in clipped] == [b"%c" % (65 + i) for i in reverse]


def tie_shape(starts, ends, std_sort):   # noqa: F811
    """Of one read's alignments in the selection's order: (alignments, those whose start an earlier one has, twice != stable, once != stable, once != twice,
    times an end moves currentEnd backwards in the twice-sorted order)."""
    starts, ends = [int(s) for s in starts], [int(e) for e in ends]
    once, twice, stable = cm.output_order(starts, std_sort, sorts=1), cm.output_order(starts, std_sort), _stable(starts)
    tied = len(starts) - len(set(starts))
    backwards = sum(ends[b] < ends[a] for a, b in zip(twice, twice[1:]))
    return len(starts), tied, twice != stable, once != stable, once != twice, backwards


def test_tier_c_has_the_ties_the_device_tests_rest_on(tmp_path, std_sort):   # noqa: F811
    """The oracle's whole-read alignments of tests/lowcomplexity.py's tier c, reads 1 to 5: more than 16 per read with tied starts, and the order after two
    std::sorts, after one and after a stable sort differ as tests/test_corrected_modes_gpu.py needs them to. A generator that drifts is noticed here."""
    import lowcomplexity as lc
    from oracle import Oracle
    g, reads, _ = lc.tier("c")
    gfa = str(tmp_path / "c.gfa")
    g.write_gfa(gfa)
    want = Oracle(gfa, long_pass=True).align(reads[:6])
    shapes = {}
    for r in range(1, 6):
        a0, a1 = int(want["read_longall_off"][r]), int(want["read_longall_off"][r + 1])
        shapes[r] = tie_shape(want["longall_start"][a0:a1], want["longall_end"][a0:a1], std_sort)
    print("read: (alignments, tied starts, twice != stable, once != stable, once != twice, ends moving backwards)", shapes)
    assert {r: s[:2] for r, s in shapes.items()} == {1: (50, 6), 2: (25, 2), 3: (23, 2), 4: (35, 20), 5: (27, 20)}
    assert {r: s[2] for r, s in shapes.items()} == {1: False, 2: False, 3: True, 4: True, 5: True}      # twice != stable
    assert {r: s[3] for r, s in shapes.items()} == {1: True, 2: True, 3: True, 4: True, 5: True}        # once != stable
    assert sum(s[4] for s in shapes.values()) >= 2 and all(s[5] >= 1 for s in shapes.values())
