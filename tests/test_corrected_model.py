"""tests/corrected_model.py on hand cases: each expected string is worked out by hand from the reference's three functions (src/GraphAligner.h:220-231,
src/ReadCorrection.cpp:22-64, src/Aligner.cpp:313-374)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import corrected_model as cm   # noqa: E402

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
