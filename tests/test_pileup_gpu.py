"""The pileup on the device (GC_COVERAGE_PILEUP; hip/gc_coverage.hip, hip/gc_pileup_core.hpp): the kernel's pileup step on traces of exact shapes
(Coverage.add_traces(seq_pos=, reads=)) against tests/pileup_model.py - rows, depth and the table byte for byte, whole and in two row ranges; what is refused before any
launch and what merges; a batch against the committed vg JSON of the same reads, however the reads are batched; chained winners, whose traces go up from the host with
their reads, in the default mode, in fast mode and without chaining; and the command's file."""
import gzip
import os
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import coverage_model as cm                                   # noqa: E402
import pileup_model as pm                                     # noqa: E402
from test_gpu_parity import gca                               # noqa: E402,F401
from test_coverage_gpu import chimeras, command, same_counts, syn   # noqa: E402,F401

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden")


def same_pileup(cov, want):
    """The handle's rows and depth against a model Pileup."""
    rows = cov.pileup_counts()
    assert rows.dtype == np.uint32 and rows.shape == (sum(want.segments.lengths), 8)
    assert np.array_equal(rows.astype(np.int64), want.flat_rows())
    same_counts(cov, want.depth)


@pytest.fixture(scope="module")
def shapes(gca, tmp_path_factory):   # noqa: F811
    """coverage_model's four segments of 1, 64, 65 and 130 bp in a chain, with pileup_model's letters (s3 holds ambiguous ones)."""
    g = pm.shape_segments()
    gfa = str(tmp_path_factory.mktemp("pileup") / "shapes.gfa")
    with open(gfa, "w") as f:
        for name, letters in zip(g.names, g.letters):
            f.write(f"S\t{name}\t{letters}\n")
        for a, b in zip(g.names, g.names[1:]):
            f.write(f"L\t{a}\t+\t{b}\t+\t0M\n")
    graph = gca.AlignmentGraph(gfa)
    assert cm.read_gfa_segments(gfa) == (pm.SHAPE_NAMES, pm.SHAPE_LENGTHS)
    return graph


def add(cov, items):
    cov.add_traces([t for t, _, _ in items], seq_pos=[q for _, q, _ in items], reads=[r for _, _, r in items])


@pytest.mark.parametrize("name", list(pm.shape_sets()))
def test_exact_shapes(gca, shapes, name):   # noqa: F811
    items = pm.shape_sets()[name]
    want = pm.shape_pileup(items)
    n = sum(pm.SHAPE_LENGTHS)
    cov = gca.Coverage(shapes, pileup=True)
    assert cov.per_base and cov.pileup
    add(cov, items)
    same_pileup(cov, want)
    assert cov.base_table() == cm.base_table(pm.SHAPE_NAMES, want.depth)
    for min_alt, fraction in ((1, 0.0), (0, 0.0), (2, 0.0), (0, 0.5), (1, 1.0)):
        text, off = cov.pileup_table(0, n, min_alt=min_alt, min_fraction=fraction, line_offsets=True)
        assert text == pm.table(want, min_alt=min_alt, min_fraction=fraction), (min_alt, fraction)
        assert [text[int(off[k]):int(off[k + 1])] for k in range(len(off) - 1)] == text.splitlines(keepends=True) and int(off[0]) == 0
    for cut in (1, 100, 129):                                  # two row ranges: the head line only in the first, the pieces join to the whole
        first, second = cov.pileup_table(0, cut), cov.pileup_table(cut, n - cut)
        assert first == pm.table(want, 0, cut) and second == pm.table(want, cut, n - cut) and first + second == pm.table(want)
    assert b"".join(text for text, _ in cov.pileup_pieces(1, 0.0, piece_bases=50)) == pm.table(want) == cov.pileup_table()
    # one trace per call, and every trace twice: every count doubles
    again = gca.Coverage(shapes, pileup=True)
    for item in items + items:
        add(again, [item])
    assert np.array_equal(again.pileup_counts().astype(np.int64), 2 * want.flat_rows())
    same_counts(again, [2 * d for d in want.depth])
    for c in (cov, again):
        c.close()


def test_what_is_refused_and_what_merges(gca, shapes):   # noqa: F811
    cases = pm.shape_cases()
    cov, other, plain = gca.Coverage(shapes, pileup=True), gca.Coverage(shapes, pileup=True), gca.Coverage(shapes, per_base=True)
    good = cases["63 cells"][0]
    with pytest.raises(RuntimeError, match="gc_coverage_add_traces2"):          # a pileup handle counts traces with their reads only
        cov.add_traces([good[0]])
    (nodes, offsets), seq_pos, read = cases["129 cells over three segments"][0]
    for bad_pos in (seq_pos[:64] + [len(read)] + seq_pos[65:], seq_pos[:-1] + [2 ** 32 - 1]):      # refused on the host, before any launch
        with pytest.raises(RuntimeError, match="seq_pos lies behind its read"):
            cov.add_traces([good[0], (nodes, offsets)], seq_pos=[good[1], bad_pos], reads=[good[2], read])
    with pytest.raises(RuntimeError, match="seq_pos lies behind its read"):
        cov.add_traces([([0], [0])], seq_pos=[[0]], reads=[b""])
    with pytest.raises(RuntimeError, match="no such node / offset"):
        cov.add_traces([([6], [130])], seq_pos=[[0]], reads=[b"A"])
    with pytest.raises(ValueError):
        cov.add_traces([good[0]], seq_pos=[good[1]])
    empty = pm.shape_pileup([])
    same_pileup(cov, empty)                                                     # a refused call counts nothing, its good traces included
    assert cov.pileup_table() == pm.HEAD.encode() and cov.pileup_table(5, 10) == b""
    with pytest.raises(RuntimeError, match="behind the table's end"):
        cov.pileup_table(sum(pm.SHAPE_LENGTHS) + 1, 1)
    with pytest.raises(RuntimeError, match="min_fraction"):
        cov.pileup_table(0, 10, min_fraction=1.5)
    with pytest.raises(RuntimeError, match="without the pileup"):
        plain.pileup_counts()
    with pytest.raises(RuntimeError, match="without the pileup"):
        plain.pileup_table(0, 10)
    # a handle without the flag: the same segment and base tables as before, through either call
    a, b = cases["both strands of s4"] + cases["the reverse strand"], cases["three traces over one base"] + cases["deletions across the chunk boundary"]
    plain.add_traces([t for t, _, _ in a])
    add(plain, b)
    old = gca.Coverage(shapes, per_base=True)
    old.add_traces([t for t, _, _ in a + b])
    both = pm.shape_pileup(a + b)
    same_counts(plain, both.depth)
    assert plain.base_table() == old.base_table() == cm.base_table(pm.SHAPE_NAMES, both.depth) and plain.segment_table() == old.segment_table() == cm.segment_table(pm.SHAPE_NAMES, both.depth)
    # a merge of two pileup handles equals one handle fed both; the source stays as it was; a pileup handle and a plain one do not merge, either way
    add(cov, a)
    add(other, b)
    cov.merge(other)
    same_pileup(cov, both)
    same_pileup(other, pm.shape_pileup(b))
    one = gca.Coverage(shapes, pileup=True)
    add(one, a + b)
    assert np.array_equal(one.pileup_counts(), cov.pileup_counts()) and one.pileup_table(0, 260, min_alt=0) == cov.pileup_table(0, 260, min_alt=0) == pm.table(both, min_alt=0)
    for x, y in ((cov, plain), (plain, cov)):
        with pytest.raises(RuntimeError, match="pileup"):
            x.merge(y)
    same_pileup(cov, both)
    # a channel that reaches 2^32 - 1 stays there, in the merge and in the kernel's own additions
    x, y = gca.Coverage(shapes, pileup=True), gca.Coverage(shapes, pileup=True)
    wrong = (([0], [0]), [0], b"-")                                             # one cell, a mismatch counted in mmN of s1's only base
    add(x, [wrong])
    add(y, [wrong])
    for _ in range(24):                                                         # Fibonacci by merging to and fro: 48 merges pass 2^32
        x.merge(y)
        y.merge(x)
    add(x, [wrong])
    rows = x.pileup_counts()
    assert int(rows[0][pm.MM_N]) == (1 << 32) - 1 and int(rows.astype(np.int64).sum()) == (1 << 32) - 1 and int(x.counts()[1][0]) == (1 << 32) - 1
    letter = pm.LETTER_OF_SET[pm.letter_set(pm.shape_letters()[0][0])]
    assert x.pileup_table(0, 1) == (pm.HEAD + f"s1\t0\t{letter}\t4294967295\t0\t0\t0\t0\t0\t4294967295\t0\t0\t0\n").encode()
    for c in (cov, other, plain, old, one, x, y):
        c.close()


# ---------------------------------------------------------------- a batch against the committed JSON; batches in flight; handles merged

@pytest.fixture(scope="module")
def syn_want(syn):   # noqa: F811
    """The yardstick is the committed file, not this run's output."""
    g = pm.Segments.from_gfa(syn.gfa)
    want = pm.Pileup(g)
    for line in open(os.path.join(GOLD, "syn20k.expected.json")).read().splitlines():
        pm.from_vg_json(line, g, into=want)
    assert want.totals() == {"mmA": 254, "mmC": 217, "mmG": 243, "mmT": 232, "mmN": 0, "del": 316, "ins_after": 306, "ins_before": 65}
    return want


def test_a_batch_equals_the_committed_json(syn, syn_want):   # noqa: F811
    gca = syn.gca   # noqa: F811
    cov = gca.Coverage(syn.graph, pileup=True)
    aligner = syn.aligner()
    out = aligner.align_batch(gca.ReadBatch(syn.reads), gaf_names=[b"r%d" % i for i in range(6)], coverage=cov)
    assert out["gaf"] == open(os.path.join(GOLD, "syn20k.expected.gaf"), "rb").read()      # counting leaves the batch's own output alone
    same_pileup(cov, syn_want)
    assert cov.pileup_table() == pm.table(syn_want) and cov.pileup_table(min_alt=0, min_fraction=0.0) == pm.table(syn_want, min_alt=0)
    assert b"".join(t for t, _ in cov.pileup_pieces(1, 0.0, piece_bases=3000)) == pm.table(syn_want)
    aligner.close()
    cov.close()


def test_three_batches_on_two_aligners_and_two_handles_merged(syn, syn_want):   # noqa: F811
    gca = syn.gca   # noqa: F811
    batches = [gca.ReadBatch(syn.reads[k:k + 2]) for k in (0, 2, 4)]
    handles = [gca.Coverage(syn.graph, pileup=True), gca.Coverage(syn.graph, pileup=True)]
    aligners = [syn.aligner(), syn.aligner()]
    for a, h in zip(aligners, handles):
        a.set_coverage(h)
    errors = []

    def work(aligner, mine):
        try:
            gca.set_device(0)
            for b in mine:
                aligner.align_batch(b)
        except BaseException as e:   # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(aligners[0], [batches[0], batches[2]])), threading.Thread(target=work, args=(aligners[1], [batches[1]]))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert int(handles[0].pileup_counts().sum()) > 0 and int(handles[1].pileup_counts().sum()) > 0
    handles[0].merge(handles[1])
    same_pileup(handles[0], syn_want)
    assert handles[0].pileup_table() == pm.table(syn_want)
    for thing in aligners + handles:
        thing.close()


# ---------------------------------------------------------------- chained winners: their traces exist on the host only, and their reads must go with them

def final_cells(kept, r):
    """(node, offset, seq_pos) lists of read r's final alignments: the chained alignment when it won, else the selected whole-read alignments."""
    if kept["chained_better"][r]:
        t = [(int(kept["read_chain_trace_off"][r]), int(kept["read_chain_trace_off"][r + 1]), "chain_trace_")]
    else:
        base = int(kept["read_longall_off"][r])
        t = [(int(kept["long_trace_off"][base + int(k)]), int(kept["long_trace_off"][base + int(k) + 1]), "long_trace_")
             for k in kept["long_index"][int(kept["read_long_off"][r]):int(kept["read_long_off"][r + 1])]]
    return [(kept[p + "node"][a:b].tolist(), kept[p + "offset"][a:b].tolist(), kept[p + "seqpos"][a:b].tolist()) for a, b, p in t]


@pytest.mark.parametrize("mode", ["default", "fast-mode", "no-colinear-chaining"])
def test_chained_winners_and_modes(gca, chimeras, mode):   # noqa: F811
    kw = {"default": {}, "fast-mode": {"fast_mode": True}, "no-colinear-chaining": {"colinear_chaining": False, "selection_method": 7}}[mode]
    graph, seeder, reads = chimeras["graph"], chimeras["seeder"], chimeras["reads"]
    g = pm.Segments.from_gfa(chimeras["gfa"])
    batch = gca.ReadBatch(reads)
    kept = gca.Aligner(graph, seeder, long_pass=True, chain_traces=1, keep_traces=2, colinear_gap=chimeras["gap"], **kw).align_batch(batch)
    flagged = (np.asarray(kept["failed_assertion"]) != 0) | (np.asarray(kept["capacity_exceeded"]) != 0)
    want, n_alignments = pm.Pileup(g), 0
    for r in range(len(reads)):
        if not flagged[r]:
            for node, offset, seq_pos in final_cells(kept, r):
                pm.from_cells(node, offset, seq_pos, reads[r], g, into=want)
                n_alignments += 1
    winners = [r for r in range(len(reads)) if kept["chained_better"][r] and not flagged[r]]
    print(mode, "chained winners:", winners, "final alignments:", n_alignments, want.totals())
    assert (len(winners) == 0) if mode == "no-colinear-chaining" else (len(winners) >= 1)
    assert sum(want.totals().values()) > 0
    cov = gca.Coverage(graph, pileup=True)
    out = gca.Aligner(graph, seeder, long_pass=True, chain_traces=0, device_output=1, colinear_gap=chimeras["gap"], **kw).align_batch(batch, coverage=cov)
    assert int(np.sum(out["out_source"])) == len(winners) and len(out["out_source"]) == n_alignments
    same_pileup(cov, want)
    assert cov.pileup_table() == pm.table(want)
    cov.close()


# ---------------------------------------------------------------- the command

def test_the_command_writes_the_table(syn, syn_want, tmp_path):   # noqa: F811
    gfa, fa = syn.gfa, tmp_path / "syn20k.fa"
    fa.write_bytes(b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(syn.reads)))
    table = pm.table(syn_want)
    command("-g", gfa, "-f", fa, "--pileup-out", tmp_path / "alone.tsv")                     # without -a
    assert (tmp_path / "alone.tsv").read_bytes() == table
    command("-g", gfa, "-f", fa, "--pileup-out", tmp_path / "p.tsv.gz", "-a", tmp_path / "o.gaf", "--base-coverage-out", tmp_path / "b.bg", "--batch-bytes", 3000, "--inflight", 2)
    packed = (tmp_path / "p.tsv.gz").read_bytes()
    assert gzip.decompress(packed) == table                                                  # (every member of the file)
    assert (tmp_path / "o.gaf").read_bytes() == open(os.path.join(GOLD, "syn20k.expected.gaf"), "rb").read()
    assert (tmp_path / "b.bg").read_bytes() == cm.base_table(syn_want.segments.names, syn_want.depth)
    command("-g", gfa, "-f", fa, "--pileup-out", tmp_path / "two.tsv", "--pileup-min-alt", 2, "--batch-bytes", 3000, "--devices", "0,0", "--inflight", 1)
    strict = (tmp_path / "two.tsv").read_bytes()
    assert strict == pm.table(syn_want, min_alt=2) and strict.count(b"\n") < table.count(b"\n")
    command("-g", gfa, "-f", fa, "--pileup-out", tmp_path / "f.tsv", "--pileup-min-alt", 0, "--pileup-min-alt-fraction", 0.5)
    assert (tmp_path / "f.tsv").read_bytes() == pm.table(syn_want, min_alt=0, min_fraction=0.5)
    assert sorted(os.listdir(tmp_path)) == ["alone.tsv", "b.bg", "f.tsv", "o.gaf", "p.tsv.gz", "syn20k.fa", "two.tsv"]      # no temporary file stays
