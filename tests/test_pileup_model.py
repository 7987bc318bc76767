"""tests/pileup_model.py: the two statements of what --pileup-out counts (the per-cell rule over traces with read positions, the edits of the vg JSON) agree on the
committed oracle results, and the hand cases pin the rule, the channels, the strands and the table with its filter."""
import json
import os

import numpy as np

import coverage_model as cm
import pileup_model as pm
from test_coverage_model import _selected_candidates

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_the_two_statements_agree_on_syn20k():
    """For each of the six output alignments at least one candidate trace of the read's selected alignment gives the rows and the depth its JSON line gives. The FASTA's
    reads are read0.., the JSON's r0..: the same reads in the same order."""
    g = pm.Segments.from_gfa(os.path.join(GOLD, "syn20k.gfa"))
    z = np.load(os.path.join(GOLD, "syn20k.expected.npz"))
    lines = open(os.path.join(GOLD, "syn20k.expected.json")).read().splitlines()
    reads = [line.strip() for line in open(os.path.join(GOLD, "syn20k.fa")) if not line.startswith(">")]
    assert len(reads) == 6 and not z["chained_better"].any()
    off = z["long_trace_off"]
    at, total, per_read = 0, pm.Pileup(g), []
    for r in range(6):
        for candidates in _selected_candidates(z, r):
            doc = json.loads(lines[at])
            at += 1
            assert doc["name"] == f"r{r}" and doc["sequence"] == reads[r]
            want = pm.from_vg_json(doc, g)
            matching = []
            for a in candidates:
                cut = slice(int(off[a]), int(off[a + 1]))
                got = pm.from_cells(z["long_trace_node"][cut], z["long_trace_offset"][cut], z["long_trace_seqpos"][cut], reads[r], g)
                if np.array_equal(got.flat_rows(), want.flat_rows()) and np.array_equal(got.flat_depth(), want.flat_depth()):
                    matching.append(a)
            assert matching, f"read {r}: no candidate trace gives the rows the JSON line's edits give"
            total.add(want)
            per_read.append(want.totals())
    assert at == len(lines) == 6
    assert total.totals() == {"mmA": 254, "mmC": 217, "mmG": 243, "mmT": 232, "mmN": 0, "del": 316, "ins_after": 306, "ins_before": 65}
    assert per_read[4]["ins_before"] == 65 and per_read[4]["ins_after"] == 0 and sum(t["ins_before"] for t in per_read) == 65      # r4 is the reverse-strand read
    # the depth is the coverage's, and at every base depth = matches + mismatches + deletions with matches >= 0
    ids = {n: i for i, n in enumerate(g.names)}
    assert np.array_equal(total.flat_depth(), cm.flat(cm.from_vg_json(lines, ids, g.lengths)))
    assert int((total.flat_depth() - total.flat_rows()[:, :pm.DEL + 1].sum(axis=1)).min()) >= 0


# ---- hand cases: segments a (ACGT), b (R), c (TTN); bigraph ids 0/1, 2/3, 4/5
G = pm.Segments(["a", "b", "c"], ["ACGT", "R", "TTN"])


def _rows(node, offset, seq_pos, read):
    p = pm.from_cells(node, offset, seq_pos, read, G)
    return p, {(s, at): {pm.CHANNELS[k]: int(v) for k, v in enumerate(row) if v} for s in range(3) for at, row in enumerate(p.rows[s]) if row.any()}


def test_every_mismatch_channel_on_the_forward_strand():
    for letter, channel in (("C", "mmC"), ("G", "mmG"), ("T", "mmT"), ("c", "mmC"), ("u", "mmT"), ("U", "mmT"), ("N", None), ("-", "mmN"), ("a", None), ("A", None)):
        _, rows = _rows([0], [0], [0], letter)              # under A
        assert rows == ({(0, 0): {channel: 1}} if channel else {}), letter
    assert _rows([0], [1], [0], "A")[1] == {(0, 1): {"mmA": 1}}   # under C
    assert _rows([0], [1], [0], "R")[1] == {(0, 1): {"mmN": 1}}   # an ambiguous read letter that does not hold C counts as mmN ...
    assert _rows([0], [1], [0], "Y")[1] == {}                     # ... and one that does is a match


def test_the_reverse_strand_complements_the_read_letter():
    # node 1 is a reversed: offset 0 is the complement of a's last letter T, an A, reported at forward position 3
    assert _rows([1], [0], [0], "A")[1] == {}
    for letter, channel in (("C", "mmG"), ("G", "mmC"), ("T", "mmA"), ("u", "mmA"), ("x", "mmN")):
        assert _rows([1], [0], [0], letter)[1] == {(0, 3): {channel: 1}}, letter
    assert _rows([1], [3], [0], "A")[1] == {(0, 0): {"mmT": 1}}   # under the complement of A: the read's A is a T on the forward strand


def test_ambiguous_graph_letters():
    assert _rows([2], [0], [0], "G")[1] == {} and _rows([2], [0], [0], "a")[1] == {}           # R holds A and G
    assert _rows([2], [0], [0], "C")[1] == {(1, 0): {"mmC": 1}}
    assert _rows([3], [0], [0], "C")[1] == {} and _rows([3], [0], [0], "A")[1] == {(1, 0): {"mmT": 1}}   # R reversed is Y
    assert _rows([4], [2], [0], "G")[1] == {} and _rows([4], [2], [0], "N")[1] == {}           # N holds everything
    assert _rows([4], [2], [0], "*")[1] == {(2, 2): {"mmN": 1}}                                # a byte that is no code matches nothing, not even N


def test_an_insertion_run_at_the_start():
    # the first cell is an aligned pair; the cells that repeat its position with new read bases are insertions behind that base
    p, rows = _rows([0, 0, 0, 0], [1, 1, 1, 2], [0, 1, 2, 3], "CAAG")
    assert rows == {(0, 1): {"ins_after": 2}} and list(p.depth[0]) == [0, 1, 1, 0]
    p, rows = _rows([1, 1, 1, 1], [1, 1, 1, 2], [0, 1, 2, 3], "CAAG")      # on the reverse strand: forward positions 2 and 1, the insertion lies before base 2
    assert rows == {(0, 2): {"ins_before": 2}} and list(p.depth[0]) == [0, 1, 1, 0]


def test_a_deletion_across_a_node_change():
    # read AR: A under a[0]; a[1..3] and b[0] deleted; R under c[0]... a T, which R (A or G) does not hold: mmN
    p, rows = _rows([0, 0, 0, 0, 2, 4], [0, 1, 2, 3, 0, 0], [0, 0, 0, 0, 0, 1], "AR")
    assert rows == {(0, 1): {"del": 1}, (0, 2): {"del": 1}, (0, 3): {"del": 1}, (1, 0): {"del": 1}, (2, 0): {"mmN": 1}}
    assert [list(d) for d in p.depth] == [[1, 1, 1, 1], [1], [1, 0, 0]]
    assert np.array_equal(p.flat_depth(), cm.flat(cm.from_traces([0, 0, 0, 0, 2, 4], [0, 1, 2, 3, 0, 0], [0, 6], G.lengths)))


def test_a_cell_that_repeats_everything_counts_nothing():
    once = _rows([0, 0], [0, 1], [0, 1], "AG")
    twice = _rows([0, 0, 0, 0], [0, 1, 1, 1], [0, 1, 1, 1], "AG")
    assert once[1] == twice[1] == {(0, 1): {"mmG": 1}} and np.array_equal(once[0].flat_depth(), twice[0].flat_depth())


def test_the_json_statement_on_a_hand_document():
    doc = {"sequence": "ACCTTCG", "path": {"mapping": [
        {"position": {"name": "a", "offset": "1"}, "edit": [{"from_length": 1, "to_length": 1, "sequence": "A"}, {"to_length": 2, "sequence": "CC"}, {"from_length": 1}, {"from_length": 1, "to_length": 1}]},
        {"position": {"name": "c", "node_id": "2", "offset": "1", "is_reverse": True}, "edit": [{"to_length": 1, "sequence": "T"}, {"from_length": 2, "to_length": 2, "sequence": "CG"}]}]}}
    p = pm.from_vg_json(doc, G)
    rows = {(s, at): {pm.CHANNELS[k]: int(v) for k, v in enumerate(row) if v} for s in range(3) for at, row in enumerate(p.rows[s]) if row.any()}
    # a[1] mismatch A, two inserted behind it, a[2] deleted, a[3] matched by T; the insertion that opens the second mapping lies behind a[3], the previous mapping's
    # last base (a forward one: ins_after); then c reversed: offsets 1, 2 are forward 1, 0, read letters C and G complemented to G and C
    assert rows == {(0, 1): {"mmA": 1, "ins_after": 2}, (0, 2): {"del": 1}, (0, 3): {"ins_after": 1}, (2, 1): {"mmG": 1}, (2, 0): {"mmC": 1}}
    assert [list(d) for d in p.depth] == [[0, 1, 1, 1], [0], [1, 1, 0]]
    # the same alignment as cells
    q = pm.from_cells([0, 0, 0, 0, 0, 0, 5, 5], [1, 1, 1, 2, 3, 3, 1, 2], [0, 1, 2, 2, 3, 4, 5, 6], "ACCTTCG", G)
    assert np.array_equal(p.flat_rows(), q.flat_rows()) and np.array_equal(p.flat_depth(), q.flat_depth())


def test_the_table_and_its_filter():
    p = pm.Pileup(G)
    for read in ("AG", "AG", "AC", "AA"):                       # a[1] = C under G, G, C, A: depth 4, mmG 2, mmA 1
        pm.from_cells([0, 0], [0, 1], [0, 1], read, G, into=p)
    pm.from_cells([5, 5], [0, 0], [0, 1], "NA", G, into=p)      # c reversed, forward 2: a match (N) and an insertion before it
    everything = pm.table(p, min_alt=0)
    assert everything == (pm.HEAD + "a\t0\tA\t4\t4\t0\t0\t0\t0\t0\t0\t0\t0\n" + "a\t1\tC\t4\t1\t1\t0\t2\t0\t0\t0\t0\t0\n" + "c\t2\tN\t1\t1\t0\t0\t0\t0\t0\t0\t1\t0\n").encode()
    assert pm.table(p, min_alt=1) == (pm.HEAD + "a\t1\tC\t4\t1\t1\t0\t2\t0\t0\t0\t0\t0\n" + "c\t2\tN\t1\t1\t0\t0\t0\t0\t0\t0\t1\t0\n").encode()
    assert pm.table(p, min_alt=2) == (pm.HEAD + "a\t1\tC\t4\t1\t1\t0\t2\t0\t0\t0\t0\t0\n").encode()
    assert pm.table(p, min_alt=3) == pm.HEAD.encode()
    # a fraction one base meets exactly: alt 2 of depth 4 at 0.5 passes, and so does alt 1 of depth 1; just above it only the latter
    assert pm.table(p, min_alt=0, min_fraction=0.5) == pm.table(p, min_alt=1)
    assert pm.table(p, min_alt=0, min_fraction=0.5000001) == (pm.HEAD + "c\t2\tN\t1\t1\t0\t0\t0\t0\t0\t0\t1\t0\n").encode()
    # row ranges: the head line only with first == 0; the pieces join to the whole
    n = sum(G.lengths)
    assert pm.table(p, 0, 2) + pm.table(p, 2, n - 2) == pm.table(p) and not pm.table(p, 2, n - 2).startswith(b"#")
    assert pm.table(pm.Pileup(pm.Segments(["", "x"], ["A", "C"])).add(pm.from_cells([0], [0], [0], "C", pm.Segments(["", "x"], ["A", "C"]))), min_alt=0) == (pm.HEAD + "0\t0\tA\t1\t0\t0\t1\t0\t0\t0\t0\t0\t0\n").encode()


def test_the_shapes_hold_what_they_claim():
    cases = pm.shape_cases()
    assert sorted({len(t[0][0]) for items in cases.values() for t in items} & {1, 63, 64, 65, 129}) == [1, 63, 64, 65, 129]
    g = pm.shape_segments()

    def kinds(item):
        (node, offset), q, _ = item
        out = []
        for i in range(len(node)):
            covers = i == 0 or (node[i], offset[i]) != (node[i - 1], offset[i - 1])
            moved = i == 0 or q[i] != q[i - 1]
            out.append("PDI."[0 if covers and moved else 1 if covers else 2 if moved else 3])
        return "".join(out)
    assert kinds(cases["deletions across the chunk boundary"][0])[58:71] == "PP" + "D" * 9 + "PP"
    assert kinds(cases["insertions across the chunk boundary"][0])[58:71] == "PP" + "I" * 9 + "PP"
    assert kinds(cases["cells that repeat altogether"][0])[62:67] == "P...P"
    lanes = pm.shape_pileup(cases["64 cells, mismatches in lanes 0 and 63"])
    assert lanes.rows[3][66][:5].sum() == 1 and lanes.rows[3][129][:5].sum() == 1 and lanes.totals()["del"] == 0
    three = pm.shape_pileup(cases["three traces over one base"])
    assert int(three.depth[2][35]) == 3 and int(three.rows[2][35][:5].sum()) == 2
    for node in (2, 3):
        item = [t for t in cases["every channel, lower case and U"] if t[0][0][0] == node]
        assert all(v > 0 for v in list(pm.shape_pileup(item).totals().values())[:5]), node
    amb = pm.shape_pileup(cases["65 cells, a whole segment with ambiguous letters"])
    assert amb.rows[2][10][1] == 1 and amb.rows[2][11].sum() == 0 and amb.rows[2][40].sum() == 0
    everything = pm.shape_pileup(pm.shape_sets()["every case"])
    assert all(v > 0 for v in everything.totals().values())
    assert int((everything.flat_depth() - everything.flat_rows()[:, :pm.DEL + 1].sum(axis=1)).min()) >= 0
    assert g.lengths == pm.SHAPE_LENGTHS
