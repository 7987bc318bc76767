"""Hand-checked cases for tests/mxm_model.py, the brute-force model the MUM / MEM seeder is held to (tests/test_mxm_host.py on the CPU, tests/test_mxm_seeds_gpu.py on the device).
Every expected list below was worked out on paper from the definitions in the model's docstring; HAND_CASES is shared with the two other files."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mxm_model as mm   # noqa: E402

# (name, {node id: segment}, read, mode, min_len, count, expected hits (node_id, node_offset, seq_pos, match_len, raw_goodness, reverse))
HAND_CASES = [
    # GATT is the segment's first four letters, ACAC its last four; nothing of the read's reverse complement AAGTGTCCAATCGG is in the segment
    ("first and last base of a segment", {10: "GATTACAC"}, "CCGATTGGACACTT", mm.MEM, 4, None, [(10, 0, 2, 4, 4, 0), (10, 4, 8, 4, 4, 0)]),
    ("the same as MUMs", {10: "GATTACAC"}, "CCGATTGGACACTT", mm.MUM, 4, None, [(10, 0, 2, 4, 4, 0), (10, 4, 8, 4, 4, 0)]),
    ("a read equal to a whole segment of min_len letters", {20: "ACGGTCAT"}, "ACGGTCAT", mm.MEM, 8, None, [(20, 0, 0, 8, 8, 0)]),
    ("a read shorter than min_len", {20: "ACGGTCAT"}, "ACGGTCA", mm.MEM, 8, None, []),
    # N equals nothing: TTGC ends at it, GGCTA starts behind it (left-maximal because x != A)
    ("N inside a read", {30: "TTGCAGGCTA"}, "TTGCNGGCTA", mm.MEM, 4, None, [(30, 5, 5, 5, 5, 0), (30, 0, 0, 4, 4, 0)]),
    # the segment is acgt$acgt: R is a separator, lower case and u are letters. The read is its own reverse complement, so every forward match (p, i) comes back on the
    # reverse strand as node_offset = 9 - off - 4, seq_pos = 8 - i - 4. Each string occurs twice: no MUM.
    ("IUPAC, lower case and U inside a segment", {40: "acguRACGT"}, "ACGTACGT", mm.MEM, 4, None,
     [(40, 0, 0, 4, 4, 0), (40, 5, 0, 4, 4, 0), (40, 0, 4, 4, 4, 0), (40, 5, 4, 4, 4, 0), (40, 5, 4, 4, 4, 1), (40, 0, 4, 4, 4, 1), (40, 5, 0, 4, 4, 1), (40, 0, 0, 4, 4, 1)]),
    ("... and no MUM, the strings being there twice", {40: "acguRACGT"}, "ACGTACGT", mm.MUM, 4, None, []),
    ("count cutting through a tie across strands", {40: "acguRACGT"}, "ACGTACGT", mm.MEM, 4, 5,
     [(40, 0, 0, 4, 4, 0), (40, 5, 0, 4, 4, 0), (40, 0, 4, 4, 4, 0), (40, 5, 4, 4, 4, 0), (40, 5, 4, 4, 4, 1)]),
    ("a string present twice forward: a MEM twice", {50: "TTGACCAGTT", 51: "GGGACCAGGG"}, "GACCAG", mm.MEM, 5, None, [(50, 2, 0, 6, 6, 0), (51, 2, 0, 6, 6, 0)]),
    ("... and no MUM", {50: "TTGACCAGTT", 51: "GGGACCAGGG"}, "GACCAG", mm.MUM, 5, None, []),
    # GTCCGT is in 60 forward, its reverse complement ACGGAC in 61 at offset 3: reverse hit at node_offset 12 - 3 - 6, seq_pos 6 - 0 - 6
    ("once forward and once as the reverse complement elsewhere: a MUM on each strand", {60: "AAGTCCGTAA", 61: "CCTACGGACTCC"}, "GTCCGT", mm.MUM, 6, None,
     [(60, 2, 0, 6, 6, 0), (61, 3, 0, 6, 6, 1)]),
    # one MEM per diagonal: those that start at the read's or the segment's first letter. (p, 0): l = min(6, 8 - p) for p = 0..4; (0, i): l = 6 - i for i = 1, 2
    ("poly-A read against poly-A segment", {70: "AAAAAAAA"}, "AAAAAA", mm.MEM, 4, None,
     [(70, 0, 0, 6, 6, 0), (70, 1, 0, 6, 6, 0), (70, 2, 0, 6, 6, 0), (70, 3, 0, 5, 5, 0), (70, 0, 1, 5, 5, 0), (70, 4, 0, 4, 4, 0), (70, 0, 2, 4, 4, 0)]),
    ("... none of them a MUM", {70: "AAAAAAAA"}, "AAAAAA", mm.MUM, 4, None, []),
    ("count cutting through a tie within a strand", {70: "AAAAAAAA"}, "AAAAAA", mm.MEM, 4, 2, [(70, 0, 0, 6, 6, 0), (70, 1, 0, 6, 6, 0)]),
    ("count larger than what exists", {70: "AAAAAAAA"}, "AAAAAA", mm.MEM, 4, 100,
     [(70, 0, 0, 6, 6, 0), (70, 1, 0, 6, 6, 0), (70, 2, 0, 6, 6, 0), (70, 3, 0, 5, 5, 0), (70, 0, 1, 5, 5, 0), (70, 4, 0, 4, 4, 0), (70, 0, 2, 4, 4, 0)]),
]


@pytest.mark.parametrize("case", HAND_CASES, ids=[c[0] for c in HAND_CASES])
def test_hand_checked(case):
    _, segments, read, mode, min_len, count, want = case
    assert mm.seeds(mm.Text(segments), read.encode(), mode, min_len, count) == want


def test_mapping_and_strands():
    assert mm.map_ref(b"ACGTacgtUuRYNn-*") == b"acgtacgttt$$$$$$"
    assert mm.map_read(b"ACGTacgtUuRYNn") == b"acgtacgtttxxxx"
    assert mm.reverse_strand(b"aacgxt") == b"axcgtt"
    text = mm.Text({3: "AC", 1: "GGN", 2: ""})
    assert text.T == b"gg$$$ac$" and text.ids == [1, 2, 3] and text.starts == [0, 4, 5, 8]   # ascending node id, a separator behind every segment, an empty segment is its separator
    assert text.locate(5) == (3, 0, 2) and text.locate(1) == (1, 1, 3)
    assert mm.read_is_flagged(b"ACGT-") and not mm.read_is_flagged(b"ACGTNRYu")
    assert mm.seeds(text, b"AC-AC", mm.MEM, 2) == []


def test_uniqueness_counts_overlapping_occurrences():
    """AAAA occurs twice in AAAAA (overlapping): bytes.count would say once."""
    text = mm.Text({1: "CAAAAAC"})
    assert not text.occurs_once(b"aaaa") and text.occurs_once(b"caaaa")
    assert mm.seeds(text, b"GAAAAG", mm.MUM, 4) == [] and len(mm.seeds(text, b"GAAAAG", mm.MEM, 4)) == 2
