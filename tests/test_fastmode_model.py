"""tests/fastmode_model.py (the chained alignment of --fast-mode, src/Aligner.cpp:409-424,834-843,880-895) on cases worked out by hand, and the C ABI's
gc_params::fast_mode: its place in the struct and its default."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from fastmode_model import fast_chained_alignment, path_to_trace   # noqa: E402

# three split nodes: 0 and 1 are the two parts of the original node 10 (5 + 4 bases), 2 is the original node 13 and holds an IUPAC letter
LENGTH = [5, 4, 6]
SEQ = ["ACGTA", "CCGT", "TTRACG"]
NODE_IDS = [10, 10, 13]
NODE_OFFSET = [0, 5, 0]


def letter(node, offset):
    return SEQ[node][offset]


def run(path, first, last, x, y, read):
    return fast_chained_alignment(path, first, last, x, y, read, LENGTH, NODE_IDS, NODE_OFFSET, letter)


def test_a_one_node_piece_runs_to_the_nodes_end():
    """pathToTrace's first branch takes the only node, so last_offset (2) is never looked at: cells 1..4 of node 0, "CGTA"."""
    assert path_to_trace([0], 1, 2, LENGTH) == [(0, 1), (0, 2), (0, 3), (0, 4)]
    node, offset, seqpos, switch, score, start, end = run([0], 1, 2, 3, 20, b"NNNCGAANNNNNNNNNNNNNNN")
    assert node == [10, 10, 10, 10]
    assert offset == [1, 2, 3, 4]
    assert seqpos == [3, 4, 5, 6]
    assert switch == [0, 0, 0, 0]
    assert score == 1                     # C=C, G=G, T/A, A=A
    assert (start, end) == (3, 7)         # the piece is shorter than y - x + 1 = 18: the end stays below y + 1 = 21


def test_a_piece_longer_than_the_chains_span_repeats_y():
    """4 cells "TACC" over x = 2, y = 4: positions 2, 3, 4, 4 - the last two cells are both compared with read[4]."""
    node, offset, seqpos, switch, score, start, end = run([0, 1], 3, 1, 2, 4, b"GGTAGG")
    assert node == [10, 10, 10, 10]
    assert offset == [3, 4, 5, 6]         # the second split node starts at offset 5 of the original node
    assert seqpos == [2, 3, 4, 4]
    assert switch == [0, 1, 0, 0]
    assert score == 2                     # T=T, A=A, C/G, C/G
    assert (start, end) == (2, 5)
    assert run([0, 1], 3, 1, 2, 4, b"GGTACG")[4] == 0


def test_two_nodes_the_last_stops_at_last_offset():
    """Node 1 from offset 2 ("GT"), node 2 up to offset 3 ("TTRA"): 6 cells, not the 8 that node 2's end would give."""
    assert path_to_trace([1, 2], 2, 3, LENGTH) == [(1, 2), (1, 3), (2, 0), (2, 1), (2, 2), (2, 3)]
    node, offset, seqpos, switch, score, start, end = run([1, 2], 2, 3, 0, 9, b"GTTTRATTTT")
    assert node == [10, 10, 13, 13, 13, 13]
    assert offset == [7, 8, 0, 1, 2, 3]
    assert seqpos == [0, 1, 2, 3, 4, 5]
    assert switch == [0, 1, 0, 0, 0, 0]
    assert score == 0                     # the read's own R equals the graph's R: chars are compared as they are
    assert (start, end) == (0, 6)


def test_an_iupac_letter_against_n_counts_as_a_difference():
    assert run([1, 2], 2, 3, 0, 9, b"GTTTNATTTT")[4] == 1          # R / N
    assert run([1, 2], 2, 3, 0, 9, b"GTTTAATTTT")[4] == 1          # R / A: no IUPAC matching either


def test_three_nodes_the_middle_one_whole():
    node, offset, seqpos, switch, score, start, end = run([0, 1, 2], 4, 0, 1, 6, b"TACCGTTA")
    assert node == [10, 10, 10, 10, 10, 13]
    assert offset == [4, 5, 6, 7, 8, 0]
    assert seqpos == [1, 2, 3, 4, 5, 6]
    assert switch == [1, 0, 0, 0, 1, 0]
    assert score == 0
    assert (start, end) == (1, 7)         # n = y - x + 1 exactly: the end is y + 1 and nothing repeats


def test_an_empty_piece_gives_no_alignment():
    assert run([], 0, 0, 0, 5, b"ACGTAC") == ([], [], [], [], 0, None, None)


def test_gc_params_has_fast_mode_in_its_tail_padding_and_off_by_default():
    """fast_mode follows selection_method in what was the struct's tail padding: no other field moves and the size stays."""
    from graphchainer_amd.api import GcParams, load_library
    lib = load_library()
    assert GcParams.fast_mode.offset == GcParams.selection_method.offset + 4
    assert GcParams.fast_mode.size == 4
    assert ctypes.sizeof(GcParams) == GcParams.fast_mode.offset + 4
    assert ctypes.sizeof(GcParams) % 8 == 0

    class Before(ctypes.Structure):        # the struct as it was
        _fields_ = GcParams._fields_[:-1]
    assert GcParams._fields_[-1][0] == "fast_mode"
    assert ctypes.sizeof(Before) == ctypes.sizeof(GcParams)
    for name, _ in Before._fields_:
        assert getattr(Before, name).offset == getattr(GcParams, name).offset, name
    p = GcParams()
    p.fast_mode, p.selection_method, p.colinear_chaining = 77, 77, 77
    lib.gc_params_default(ctypes.byref(p))
    assert p.fast_mode == 0
    assert (p.selection_method, p.colinear_chaining, p.chain_traces, p.stitch, p.edit_distances) == (0, 1, 1, 1, 1)
