"""tests/coverage_model.py: the two statements of what --coverage-out / --base-coverage-out count (the per-cell rule over traces, the mapping intervals of the vg JSON)
agree on the committed oracle results, and the hand cases pin the rule and the two file formats."""
import json
import os

import numpy as np

import coverage_model as cm

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _graph(name):
    names, lengths = cm.read_gfa_segments(os.path.join(GOLD, name))
    return names, lengths, {n: i for i, n in enumerate(names)}


def _selected_candidates(z, r):
    """The fixture holds the trace of every whole-read alignment of a read and the (start, end, score) of the selected ones, not their indices: the candidates of a
    selected alignment are the read's alignments with its triple (several alignments of a read can share one, test_oracle_golden.py)."""
    out = []
    for k in range(int(z["read_long_off"][r]), int(z["read_long_off"][r + 1])):
        key = (int(z["long_start"][k]), int(z["long_end"][k]), int(z["long_score"][k]))
        out.append([a for a in range(int(z["read_longall_off"][r]), int(z["read_longall_off"][r + 1]))
                    if (int(z["longall_start"][a]), int(z["longall_end"][a]), int(z["longall_score"][a])) == key])
    return out


def test_the_two_statements_agree_on_syn20k():
    """No chained alignment wins in this fixture, so the JSON's lines are the selected whole-read alignments, one per read, in read order. Every line's mapping intervals
    equal the per-cell rule over a candidate trace of that read's selected alignment (r0 and r2: both candidates give the same depth; r4: the first of two does)."""
    names, lengths, ids = _graph("syn20k.gfa")
    z = np.load(os.path.join(GOLD, "syn20k.expected.npz"))
    lines = open(os.path.join(GOLD, "syn20k.expected.json")).read().splitlines()
    assert not z["chained_better"].any() and not z["failed_assertion"].any()
    off = z["long_trace_off"]
    at, total = 0, [np.zeros(n, dtype=np.int64) for n in lengths]
    for r in range(len(z["chained_better"])):
        for candidates in _selected_candidates(z, r):
            assert candidates
            want = cm.from_vg_json([lines[at]], ids, lengths)
            assert json.loads(lines[at])["name"] == f"r{r}"
            at += 1
            matching = []
            for a in candidates:
                got = cm.from_traces(z["long_trace_node"][off[a]:off[a + 1]], z["long_trace_offset"][off[a]:off[a + 1]], [0, int(off[a + 1] - off[a])], lengths)
                if np.array_equal(cm.flat(got), cm.flat(want)):
                    matching.append(a)
            assert matching, f"read {r}: no candidate trace covers what the JSON line's mappings cover"
            total = [t + w for t, w in zip(total, want)]
    assert at == len(lines) == 6
    assert np.array_equal(cm.flat(total), cm.flat(cm.from_vg_json(lines, ids, lengths)))
    assert int(cm.bases_of(total).sum()) == 1996 + 2008 + 1981 + 1987 + 1988 + 1985
    # r4 lies on the reverse strand: its bases are reported in forward coordinates of segments the forward reads cover too
    assert max(int(d.max()) for d in total if len(d)) >= 2


def test_the_two_statements_agree_on_ref_test():
    names, lengths, ids = _graph("ref_test_graph.gfa")
    z = np.load(os.path.join(GOLD, "ref_test.expected.npz"))
    doc = json.load(open(os.path.join(GOLD, "ref_test.expected.gam.json")))
    assert len(z["long_trace_off"]) == 2 and list(z["chained_better"]) == [0]      # one read, one alignment: it is the selected one
    got = cm.from_traces(z["long_trace_node"], z["long_trace_offset"], z["long_trace_off"], lengths)
    want = cm.from_vg_json([aln for group in doc["groups"] for aln in group], ids, lengths)
    assert np.array_equal(cm.flat(got), cm.flat(want)) and int(cm.flat(got).sum()) == 70
    assert cm.segment_table(names, got).decode().splitlines()[0] == "#segment\tlength\tbases"
    assert [line.split("\t")[0] for line in cm.base_table(names, got).decode().splitlines()] == ["1", "2", "4"]      # the read goes through segment 2, not 3


# ---- hand cases: segments a (4 bp), b (1 bp), c (3 bp); bigraph ids 0/1, 2/3, 4/5
NAMES, LENGTHS = ["a", "b", "c"], [4, 1, 3]


def _depth(traces):
    node = [n for t in traces for n, _ in t]
    offset = [o for t in traces for _, o in t]
    off = np.concatenate([[0], np.cumsum([len(t) for t in traces])])
    return [list(map(int, d)) for d in cm.from_traces(node, offset, off, LENGTHS)]


def test_one_cell():
    assert _depth([[(0, 2)]]) == [[0, 0, 1, 0], [0], [0, 0, 0]]


def test_an_insertion_at_the_start_covers_once():
    # the first cell always covers; the cells that repeat its position are read bases without a graph base
    assert _depth([[(0, 1), (0, 1), (0, 1), (0, 2)]]) == [[0, 1, 1, 0], [0], [0, 0, 0]]


def test_a_deletion_covers_every_base_it_passes():
    # three graph bases under one read position are three cells with their own offsets (seqPos, which the rule does not read, stands still)
    assert _depth([[(0, 0), (0, 1), (0, 2), (0, 3)]]) == [[1, 1, 1, 1], [0], [0, 0, 0]]


def test_a_reverse_strand_node_is_flipped():
    assert _depth([[(5, 0), (5, 1)]]) == [[0, 0, 0, 0], [0], [0, 1, 1]]
    assert _depth([[(1, 3)]]) == [[1, 0, 0, 0], [0], [0, 0, 0]]


def test_a_segment_of_length_one_on_both_strands():
    assert _depth([[(2, 0)], [(3, 0)]]) == [[0, 0, 0, 0], [2], [0, 0, 0]]


def test_two_alignments_over_one_base_and_the_tables():
    depth = cm.from_traces(*zip(*[(0, 1), (0, 2), (2, 0), (4, 0), (0, 2), (0, 3)]), [0, 4, 6], LENGTHS)
    assert [list(map(int, d)) for d in depth] == [[0, 1, 2, 1], [1], [1, 0, 0]]
    assert cm.segment_table(NAMES, depth) == b"#segment\tlength\tbases\na\t4\t4\nb\t1\t1\nc\t3\t1\n"
    # a run ends where the depth changes and at a segment's end, equal depths on both sides or not
    assert cm.base_table(NAMES, depth) == b"a\t1\t2\t1\na\t2\t3\t2\na\t3\t4\t1\nb\t0\t1\t1\nc\t0\t1\t1\n"
    assert cm.segment_table(["", "x", ""], depth).splitlines()[1:] == [b"0\t4\t4", b"x\t1\t1", b"2\t3\t1"]      # a segment without a name prints its number


def test_the_same_position_on_another_node_covers():
    # offset 0 of node 2 after offset 0 of node 0: another node, so a new base, whatever the offsets say
    assert _depth([[(0, 0), (2, 0)]]) == [[1, 0, 0, 0], [1], [0, 0, 0]]


def test_a_mapping_without_offset_or_edits_and_a_reverse_mapping():
    ids = {n: i for i, n in enumerate(NAMES)}
    doc = {"path": {"mapping": [{"position": {"name": "a", "offset": "1"}, "edit": [{"from_length": 2, "to_length": 2}, {"to_length": 3, "sequence": "AAA"}, {"from_length": 1}]},
                                {"position": {"name": "c", "node_id": "2", "is_reverse": True}, "edit": [{"from_length": 2, "to_length": 2}]}]}}
    assert [list(map(int, d)) for d in cm.from_vg_json([doc, json.dumps({"name": "unaligned"})], ids, LENGTHS)] == [[0, 1, 1, 1], [0], [0, 1, 1]]
