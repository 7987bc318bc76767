"""Coverage on the device (gc_coverage_*; hip/gc_coverage.hip): the kernels on traces of exact shapes (Coverage.add_traces) against tests/coverage_model.py - counts and
both tables byte for byte; a batch against the committed vg JSON of the same reads; the same counts however the reads are batched, over two aligners sharing a handle
and over two handles merged; chained winners, whose traces go up from the host, in the default mode, in fast mode and without chaining; and the command's two files."""
import gzip
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import coverage_model as cm                                   # noqa: E402
from test_gpu_parity import gca                               # noqa: E402,F401

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden")
SHAPE_NAMES = ["s1", "s2", "s3", "s4"]


def same_counts(cov, depth):
    """The handle's counts and both tables against a model depth (one array per segment); names from the handle's graph file."""
    bases, got = cov.counts()
    assert bases.dtype == np.uint64 and np.array_equal(bases, cm.bases_of(depth))
    if cov.per_base:
        assert got.dtype == np.uint32 and np.array_equal(got.astype(np.int64), cm.flat(depth))
    else:
        assert got is None


@pytest.fixture(scope="module")
def shapes(gca, tmp_path_factory):   # noqa: F811
    """Four segments of 1, 64, 65 and 130 bp in a chain; the last one is three split nodes."""
    rng = np.random.default_rng(3)
    gfa = str(tmp_path_factory.mktemp("coverage") / "shapes.gfa")
    with open(gfa, "w") as f:
        for name, n in zip(SHAPE_NAMES, cm.SHAPE_LENGTHS):
            f.write(f"S\t{name}\t" + bytes(rng.choice(list(b"ACGT"), size=n).tolist()).decode() + "\n")
        for a, b in zip(SHAPE_NAMES, SHAPE_NAMES[1:]):
            f.write(f"L\t{a}\t+\t{b}\t+\t0M\n")
    graph = gca.AlignmentGraph(gfa)
    assert cm.read_gfa_segments(gfa) == (SHAPE_NAMES, cm.SHAPE_LENGTHS) and int(np.sum(graph.array("nodeLength"))) == 2 * sum(cm.SHAPE_LENGTHS)
    assert int(np.sum(graph.array("nodeIDs") == 6)) == 3
    return graph


@pytest.mark.parametrize("name", list(cm.shape_sets()))
def test_exact_shapes(gca, shapes, name):   # noqa: F811
    traces = cm.shape_sets()[name]
    depth = cm.traces_depth(traces)
    cov = gca.Coverage(shapes, per_base=True)
    cov.add_traces(traces)
    same_counts(cov, depth)
    segments, seg_off = cov.segment_table(line_offsets=True)
    runs, run_off = cov.base_table(line_offsets=True)
    assert segments == cm.segment_table(SHAPE_NAMES, depth)
    assert runs == cm.base_table(SHAPE_NAMES, depth)
    for text, off in ((segments, seg_off), (runs, run_off)):   # the offsets cut the text into its lines
        assert [text[int(off[k]):int(off[k + 1])] for k in range(len(off) - 1)] == text.splitlines(keepends=True) and int(off[0]) == 0
    # one trace per call, and every trace twice: depths double, the runs stay where they are
    again = gca.Coverage(shapes, per_base=True)
    for t in traces + traces:
        again.add_traces([t])
    same_counts(again, [2 * d for d in depth])
    assert again.base_table() == cm.base_table(SHAPE_NAMES, [2 * d for d in depth])
    # without the per-base depth: the same bases, no depth, no base table
    plain = gca.Coverage(shapes)
    plain.add_traces(traces)
    same_counts(plain, depth)
    assert plain.segment_table() == segments
    with pytest.raises(RuntimeError, match="without per-base depth"):
        plain.base_table()
    for c in (cov, again, plain):
        c.close()


def test_what_is_refused_and_what_merges(gca, shapes):   # noqa: F811
    cases = cm.shape_cases()
    cov, other, plain = gca.Coverage(shapes, per_base=True), gca.Coverage(shapes, per_base=True), gca.Coverage(shapes)
    for bad in (([6], [130]), ([8], [0]), ([-1], [0]), ([0, 1], [0, 1])):   # an offset behind its segment, no such node, the second cell of a trace
        with pytest.raises(RuntimeError, match="no such node / offset"):
            cov.add_traces([cases["63 cells"][0], bad])
    same_counts(cov, cm.traces_depth([]))                                    # a refused call counts nothing, its good traces included
    cov.add_traces([])
    cov.add_traces([([], [])])
    same_counts(cov, cm.traces_depth([]))
    assert cov.base_table() == b"" and cov.segment_table() == cm.segment_table(SHAPE_NAMES, cm.traces_depth([]))
    cov.add_traces(cases["both strands of s4"])
    other.add_traces(cases["depth three"] + cases["the reverse strand"])
    cov.merge(other)
    merged = cm.traces_depth(cases["both strands of s4"] + cases["depth three"] + cases["the reverse strand"])
    same_counts(cov, merged)
    same_counts(other, cm.traces_depth(cases["depth three"] + cases["the reverse strand"]))       # the source stays as it was
    assert cov.base_table() == cm.base_table(SHAPE_NAMES, merged)
    with pytest.raises(RuntimeError, match="per base"):
        cov.merge(plain)
    with pytest.raises(RuntimeError, match="itself"):
        cov.merge(cov)
    elsewhere = gca.AlignmentGraph(os.path.join(GOLD, "ref_test_graph.gfa"))
    foreign = gca.Coverage(elsewhere, per_base=True)
    with pytest.raises(RuntimeError, match="different shape"):
        cov.merge(foreign)
    # a depth word that reaches 2^32 - 1 stays there, in the merge and in the kernel's own additions; bases, 64 bits wide, goes on counting
    x, y = gca.Coverage(shapes, per_base=True), gca.Coverage(shapes, per_base=True)
    x.add_traces([([0], [0])])
    y.add_traces([([0], [0])])
    a, b = 1, 1
    for _ in range(24):                      # Fibonacci by merging to and fro: 48 merges pass 2^32
        x.merge(y)
        a += b
        y.merge(x)
        b += a
    assert a > 1 << 32 and b < 1 << 63
    x.add_traces([([0], [0]), ([1], [0])])
    bases, depth = x.counts()
    assert int(bases[0]) == a + 2 and int(depth[0]) == (1 << 32) - 1 and int(depth[1:].sum()) == 0
    assert x.base_table() == b"s1\t0\t1\t4294967295\n" and x.segment_table().splitlines()[1] == b"s1\t1\t%d" % (a + 2)
    for c in (cov, other, plain, foreign, x, y):
        c.close()


# ---------------------------------------------------------------- a batch against the committed JSON; batches in flight; handles merged

class Syn20k:
    def __init__(self, gca):   # noqa: F811
        self.gfa = os.path.join(GOLD, "syn20k.gfa")
        self.reads = [line.strip().encode() for line in open(os.path.join(GOLD, "syn20k.fa")) if not line.startswith(">")]
        self.names, self.lengths = cm.read_gfa_segments(self.gfa)
        ids = {n: i for i, n in enumerate(self.names)}
        # the yardstick is the committed file, not this run's output
        self.want = cm.from_vg_json(open(os.path.join(GOLD, "syn20k.expected.json")).read().splitlines(), ids, self.lengths)
        self.graph = gca.AlignmentGraph(self.gfa)
        self.seeder = gca.MinimizerSeeder(self.graph)
        self.gca = gca

    def aligner(self, **kw):
        return self.gca.Aligner(self.graph, self.seeder, long_pass=True, device_output=1, **kw)


@pytest.fixture(scope="module")
def syn(gca):   # noqa: F811
    return Syn20k(gca)


def test_a_batch_equals_the_committed_json(syn):
    gca = syn.gca   # noqa: F811
    assert len(syn.reads) == 6 and sum(syn.lengths) >= 20000 and int(cm.flat(syn.want).sum()) > 11000
    cov = gca.Coverage(syn.graph, per_base=True)
    aligner = syn.aligner()
    batch = gca.ReadBatch(syn.reads)
    names = [b"r%d" % i for i in range(6)]
    out = aligner.align_batch(batch, gaf_names=names, coverage=cov)
    assert out["gaf"] == open(os.path.join(GOLD, "syn20k.expected.gaf"), "rb").read()      # counting leaves the batch's own output alone
    same_counts(cov, syn.want)
    assert cov.segment_table() == cm.segment_table(syn.names, syn.want) and cov.base_table() == cm.base_table(syn.names, syn.want)
    assert aligner.coverage is None
    aligner.align_batch(batch)                                                              # the handle was set for that one call
    same_counts(cov, syn.want)
    aligner.set_coverage(cov)
    aligner.align_batch(batch)
    same_counts(cov, [2 * d for d in syn.want])
    with pytest.raises(ValueError):
        gca.Aligner(syn.graph, syn.seeder, long_pass=True).align_batch(batch, coverage=cov)
    aligner.close()
    cov.close()


def test_three_batches_on_two_aligners_and_two_handles_merged(syn):
    gca = syn.gca   # noqa: F811
    batches = [gca.ReadBatch(syn.reads[k:k + 2]) for k in (0, 2, 4)]
    shared = gca.Coverage(syn.graph, per_base=True)
    aligners = [syn.aligner(), syn.aligner()]
    for a in aligners:
        a.set_coverage(shared)
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
    same_counts(shared, syn.want)
    assert shared.base_table() == cm.base_table(syn.names, syn.want)
    # two halves on two handles, merged afterwards
    first, second = gca.Coverage(syn.graph, per_base=True), gca.Coverage(syn.graph, per_base=True)
    halves = [gca.ReadBatch(syn.reads[:3]), gca.ReadBatch(syn.reads[3:])]
    aligners[0].align_batch(halves[0], coverage=first)
    aligners[1].align_batch(halves[1], coverage=second)
    assert int(first.counts()[0].sum()) > 0 and int(second.counts()[0].sum()) > 0
    first.merge(second)
    same_counts(first, syn.want)
    assert first.segment_table() == shared.segment_table() and first.base_table() == shared.base_table()
    for thing in aligners + [shared, first, second]:
        thing.close()


# ---------------------------------------------------------------- chained winners: their traces exist on the host only

@pytest.fixture(scope="module")
def chimeras(gca, tmp_path_factory):   # noqa: F811
    """The graph and reads of tests/test_fast_mode_gpu.py (a chimera whose chain is cut at --colinear-gap 200, junk the whole-read pass cannot cross): chained winners."""
    from graphchainer_amd.synth import SynthGraph
    from test_fast_mode_gpu import GAP, make_reads
    sg = SynthGraph(40_000, seed=23, repeats=3)
    gfa = str(tmp_path_factory.mktemp("chimeras") / "g.gfa")
    sg.write_gfa(gfa)
    graph = gca.AlignmentGraph(gfa)
    return {"gfa": gfa, "graph": graph, "seeder": gca.MinimizerSeeder(graph), "reads": make_reads(sg)[0], "gap": GAP}


def final_traces(kept, r):
    """(node, offset) lists of read r's final alignments: the chained alignment when it won, else the selected whole-read alignments."""
    if kept["chained_better"][r]:
        t = [(int(kept["read_chain_trace_off"][r]), int(kept["read_chain_trace_off"][r + 1]), "chain_trace_")]
    else:
        base = int(kept["read_longall_off"][r])
        t = [(int(kept["long_trace_off"][base + int(k)]), int(kept["long_trace_off"][base + int(k) + 1]), "long_trace_")
             for k in kept["long_index"][int(kept["read_long_off"][r]):int(kept["read_long_off"][r + 1])]]
    return [(kept[p + "node"][a:b].tolist(), kept[p + "offset"][a:b].tolist()) for a, b, p in t]


@pytest.mark.parametrize("mode", ["default", "fast-mode", "no-colinear-chaining"])
def test_chained_winners_and_modes(gca, chimeras, mode):   # noqa: F811
    kw = {"default": {}, "fast-mode": {"fast_mode": True}, "no-colinear-chaining": {"colinear_chaining": False, "selection_method": 7}}[mode]
    graph, seeder, reads = chimeras["graph"], chimeras["seeder"], chimeras["reads"]
    names, lengths = cm.read_gfa_segments(chimeras["gfa"])
    batch = gca.ReadBatch(reads)
    kept = gca.Aligner(graph, seeder, long_pass=True, chain_traces=1, keep_traces=2, colinear_gap=chimeras["gap"], **kw).align_batch(batch)
    flagged = (np.asarray(kept["failed_assertion"]) != 0) | (np.asarray(kept["capacity_exceeded"]) != 0)
    traces = [t for r in range(len(reads)) if not flagged[r] for t in final_traces(kept, r)]
    winners = [r for r in range(len(reads)) if kept["chained_better"][r] and not flagged[r]]
    print(mode, "chained winners:", winners, "final alignments:", len(traces))
    assert (len(winners) == 0) if mode == "no-colinear-chaining" else (len(winners) >= 1)
    want = cm.traces_depth(traces, lengths)
    cov = gca.Coverage(graph, per_base=True)
    # chain_traces=0: the winners' traces are made for the counting all the same
    out = gca.Aligner(graph, seeder, long_pass=True, chain_traces=0, device_output=1, colinear_gap=chimeras["gap"], **kw).align_batch(batch, coverage=cov)
    assert int(np.sum(out["out_source"])) == len(winners) and len(out["out_source"]) == len(traces)
    same_counts(cov, want)
    assert cov.base_table() == cm.base_table(names, want) and cov.segment_table() == cm.segment_table(names, want)
    cov.close()


# ---------------------------------------------------------------- the command

def command(*args):
    out = subprocess.run([sys.executable, "-m", "graphchainer_amd"] + [str(a) for a in args], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout + out.stderr
    return out


def test_the_command_writes_both_tables(syn, tmp_path):
    # the reads of tests/golden/syn20k.fa under the ids the golden GAF was written with (the file's own are read0 ..): o.gaf can then be held to it byte for byte
    gfa, fa = syn.gfa, tmp_path / "syn20k.fa"
    fa.write_bytes(b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(syn.reads)))
    segments, runs = cm.segment_table(syn.names, syn.want), cm.base_table(syn.names, syn.want)
    command("-g", gfa, "-f", fa, "--coverage-out", tmp_path / "c.tsv", "--base-coverage-out", tmp_path / "b.bg.gz", "-a", tmp_path / "o.gaf")
    assert (tmp_path / "c.tsv").read_bytes() == segments
    assert gzip.decompress((tmp_path / "b.bg.gz").read_bytes()) == runs
    assert (tmp_path / "o.gaf").read_bytes() == open(os.path.join(GOLD, "syn20k.expected.gaf"), "rb").read()      # nothing else moved
    command("-g", gfa, "-f", fa, "--coverage-out", tmp_path / "alone.tsv.gz", "--base-coverage-out", tmp_path / "alone.bg")
    assert gzip.decompress((tmp_path / "alone.tsv.gz").read_bytes()) == segments and (tmp_path / "alone.bg").read_bytes() == runs
    command("-g", gfa, "-f", fa, "--coverage-out", tmp_path / "small.tsv", "--base-coverage-out", tmp_path / "small.bg.gz", "--batch-bytes", 3000, "--inflight", 2)
    assert (tmp_path / "small.tsv").read_bytes() == segments and gzip.decompress((tmp_path / "small.bg.gz").read_bytes()) == runs
    # two replicas (the one device named twice): a handle each, merged into the first before the tables are written
    command("-g", gfa, "-f", fa, "--coverage-out", tmp_path / "two.tsv", "--base-coverage-out", tmp_path / "two.bg", "--batch-bytes", 3000, "--devices", "0,0", "--inflight", 1)
    assert (tmp_path / "two.tsv").read_bytes() == segments and (tmp_path / "two.bg").read_bytes() == runs
    assert sorted(os.listdir(tmp_path)) == ["alone.bg", "alone.tsv.gz", "b.bg.gz", "c.tsv", "o.gaf", "small.bg.gz", "small.tsv", "syn20k.fa", "two.bg", "two.tsv"]      # no temporary file stays
