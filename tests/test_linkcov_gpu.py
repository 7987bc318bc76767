"""Link coverage on the device (gc_coverage_create2 with GC_COVERAGE_LINKS; hip/gc_coverage.hip): the traversal step of k_cov_add on traces of exact shapes
(Coverage.add_traces) against tests/link_coverage_model.py - counts, the link table and the tagged GFA byte for byte; what is refused; the merge; and the command's three
files on the graph and reads of tests/test_coverage_gpu.py (chained winners among them), held to the model over the GAF the same run writes."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import coverage_model as cm                                   # noqa: E402
import link_coverage_model as lm                              # noqa: E402
from test_gpu_parity import gca                               # noqa: E402,F401

pytestmark = pytest.mark.gpu
LINKS = lm.graph_links()


@pytest.fixture(scope="module")
def hand(gca, tmp_path_factory):   # noqa: F811
    """link_coverage_model's graph: six segments of 1, 63, 64, 65, 130 and 7 bp, a side road over a reverse strand, a hairpin. Lower-case letters, U and IUPAC codes in
    the file: the tagged GFA spells them as the graph holds them."""
    gfa = str(tmp_path_factory.mktemp("linkcov") / "hand.gfa")
    letters = lm.write_graph(gfa)
    letters[4] = letters[4][:70] + "R" + letters[4][71:129] + "n"
    letters[5] = "acguNyK"
    text = open(gfa).read().splitlines(keepends=True)
    for i in (4, 5):
        text[i] = f"S\t{lm.NAMES[i]}\t{letters[i]}\n"
    open(gfa, "w").write("".join(text))
    graph = gca.AlignmentGraph(gfa)
    assert lm.links_of_gfa(gfa) == LINKS and cm.read_gfa_segments(gfa) == (lm.NAMES, lm.LENGTHS)
    return {"graph": graph, "letters": [s.upper().replace("U", "T") for s in letters]}


def same_links(cov, counts):
    src, dst, got = cov.link_counts()
    assert src.dtype == np.int32 and got.dtype == np.uint64
    assert list(zip(src.tolist(), dst.tolist())) == LINKS and got.tolist() == [counts.get(k, 0) for k in LINKS]


def whole_gfa(cov, **kw):
    return b"".join(text for text, _ in cov.gfa_pieces(**kw))


@pytest.mark.parametrize("name", list(lm.cases()) + ["every case"])
def test_exact_shapes(gca, hand, name):   # noqa: F811
    traces = lm.every_case() if name == "every case" else lm.cases()[name]
    counts, depth = lm.from_traces(traces), cm.traces_depth(traces, lm.LENGTHS)
    cov = gca.Coverage(hand["graph"], per_base=True, links=True)
    cov.add_traces(traces)
    same_links(cov, counts)
    bases, got_depth = cov.counts()
    assert np.array_equal(bases, cm.bases_of(depth)) and np.array_equal(got_depth.astype(np.int64), cm.flat(depth))
    table, off = cov.link_table(line_offsets=True)
    assert table == lm.link_table(lm.NAMES, LINKS, counts)
    assert [table[int(off[k]):int(off[k + 1])] for k in range(len(off) - 1)] == table.splitlines(keepends=True) and int(off[0]) == 0
    for kept in (False, True):
        want = lm.gfa_text(lm.NAMES, hand["letters"], bases, LINKS, counts, supported_only=kept)
        assert whole_gfa(cov, supported_only=kept) == want
        # piece by piece - a row per call - the same text, every piece whole lines
        pieces = list(cov.gfa_pieces(supported_only=kept, piece_bytes=1))
        assert b"".join(t for t, _ in pieces) == want and len(pieces) == 1 + len(lm.NAMES) + len(LINKS)
        for text, line_off in pieces:
            assert [text[int(line_off[k]):int(line_off[k + 1])] for k in range(len(line_off) - 1)] == text.splitlines(keepends=True)
        segments, links = lm.read_tagged_gfa(want)
        for a, _, b, _, overlap, rc in links:      # a kept link has both ends kept: a traversal covers a base on either side
            assert overlap == "0M" and (not kept or (rc > 0 and a in segments and b in segments))
    assert b"".join(t for t, _ in cov.link_pieces(piece_bytes=1)) == table
    # the same traces one call each, twice over: every count doubles
    again = gca.Coverage(hand["graph"], links=True)
    for t in traces + traces:
        again.add_traces([t])
    same_links(again, {k: 2 * v for k, v in counts.items()})
    # a handle without links: bases and depth as ever, and nothing of the rest
    plain = gca.Coverage(hand["graph"], per_base=True)
    plain.add_traces(traces)
    plain_bases, plain_depth = plain.counts()
    assert np.array_equal(plain_bases, bases) and np.array_equal(plain_depth, got_depth) and plain.segment_table() == cov.segment_table() and plain.base_table() == cov.base_table()
    with pytest.raises(RuntimeError, match="without links"):
        plain.link_table()
    for c in (cov, again, plain):
        c.close()


def test_what_is_refused_and_what_merges(gca, hand):   # noqa: F811
    cases = lm.cases()
    cov, other, plain = gca.Coverage(hand["graph"], per_base=True, links=True), gca.Coverage(hand["graph"], per_base=True, links=True), gca.Coverage(hand["graph"], per_base=True)
    cov.add_traces(cases["the side road"])
    before = lm.from_traces(cases["the side road"])
    bases_before, depth_before = cov.counts()
    good = cases["a traversal at cell 63"][0]
    refused = {"along no link": [([0, 4], [0, 0]),                       # a+ -> c+: both offsets right, no such link
                                 ([9, 8], [129, 0]),                     # e- -> e+: the hairpin runs the other way only
                                 ([2, 10], [62, 0])],                    # b+ -> f+: the link enters f's reverse strand
               "last base": [([2, 4], [5, 0]),                           # leaves b before its last base
                             ([2, 4], [62, 1]),                          # enters c behind its first base
                             ([5, 3], [62, 0])]}                         # c- has 64 bases: 62 is not its last
    for why, traces in refused.items():
        for bad in traces:
            with pytest.raises(RuntimeError, match=why):
                cov.add_traces([good, bad])
            plain.add_traces([bad])                                      # a handle without links takes them as before: every cell lies in the graph
    same_links(cov, before)                                              # a refused call counts nothing, its good trace included, segments included
    bases, depth = cov.counts()
    assert np.array_equal(bases, bases_before) and np.array_equal(depth, depth_before)
    # merge: two handles equal one handle fed both; the source stays as it was
    other.add_traces(cases["the hairpin"] + cases["one link on both strands"])
    cov.merge(other)
    both = cases["the side road"] + cases["the hairpin"] + cases["one link on both strands"]
    same_links(cov, lm.from_traces(both))
    same_links(other, lm.from_traces(cases["the hairpin"] + cases["one link on both strands"]))
    one = gca.Coverage(hand["graph"], per_base=True, links=True)
    one.add_traces(both)
    assert one.link_table() == cov.link_table() and whole_gfa(one) == whole_gfa(cov) and one.base_table() == cov.base_table()
    with pytest.raises(RuntimeError, match="counts links"):
        cov.merge(plain)
    with pytest.raises(RuntimeError, match="counts links"):
        plain.merge(cov)
    same_links(cov, lm.from_traces(both))
    for c in (cov, other, plain, one):
        c.close()


# ---------------------------------------------------------------- the command

def command(*args):
    out = subprocess.run([sys.executable, "-m", "graphchainer_amd"] + [str(a) for a in args], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout + out.stderr
    return out


def test_the_command_writes_the_link_table_and_both_graphs(gca, tmp_path):   # noqa: F811
    from graphchainer_amd.synth import SynthGraph
    from test_fast_mode_gpu import GAP, make_reads
    sg = SynthGraph(40_000, seed=23, repeats=3)                 # the graph and reads of test_coverage_gpu.py's chained winners
    gfa, fa = str(tmp_path / "g.gfa"), tmp_path / "reads.fa"
    sg.write_gfa(gfa)
    reads = make_reads(sg)[0]
    fa.write_bytes(b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(reads)))
    names, lengths = cm.read_gfa_segments(gfa)
    ids, links = lm.segment_ids_of_gfa(gfa), lm.links_of_gfa(gfa)
    letters = {}
    for line in open(gfa):
        f = line.rstrip("\n").split("\t")
        if f[0] == "S":
            letters[f[1]] = f[2].upper()
    graph = gca.AlignmentGraph(gfa)
    out = gca.Aligner(graph, gca.MinimizerSeeder(graph), long_pass=True, device_output=1, colinear_gap=GAP).align_batch(gca.ReadBatch(reads))
    assert int(np.sum(out["out_source"])) >= 1                  # reads whose chained alignment wins are among them

    def check(d):
        gaf = (d / "o.gaf").read_text()
        counts = lm.from_gaf(gaf, ids)
        assert len(gaf.splitlines()) >= len(reads) - 1 and sum(counts.values()) > 10 and set(counts) <= set(links)
        assert (d / "l.tsv").read_bytes() == lm.link_table(names, links, counts)
        table = (d / "c.tsv").read_text().splitlines()[1:]
        bases = [int(row.split("\t")[2]) for row in table]
        assert [row.split("\t")[0] for row in table] == names
        whole = gzip.decompress((d / "g.gfa.gz").read_bytes())
        assert whole == lm.gfa_text(names, [letters[n] for n in names], bases, links, counts)
        segments, rows = lm.read_tagged_gfa(whole)
        assert list(segments) == names and [s[0] for s in segments.values()] == [letters[n] for n in names] and [s[1] for s in segments.values()] == lengths
        assert [s[2] for s in segments.values()] == bases                                                       # RC on a segment: the segment table's bases
        assert [lm.canonical(2 * ids[a] + (ao == "-"), 2 * ids[b] + (bo == "-")) for a, ao, b, bo, _, _ in rows] == links      # the input's link set, in link order
        assert [r[5] for r in rows] == [counts.get(k, 0) for k in links]                                        # RC on a link: the link table's traversals
        kept = (d / "s.gfa").read_bytes()
        assert kept == lm.gfa_text(names, [letters[n] for n in names], bases, links, counts, supported_only=True)
        kept_segments, kept_rows = lm.read_tagged_gfa(kept)
        assert list(kept_segments) == [n for n, b in zip(names, bases) if b > 0] and 0 < len(kept_segments) < len(names)      # exactly the rows with non-zero counts
        assert [r[5] for r in kept_rows] == [counts[k] for k in links if counts.get(k, 0) > 0] and 0 < len(kept_rows) < len(links)
        for a, _, b, _, _, _ in kept_rows:
            assert a in kept_segments and b in kept_segments                                                    # every kept link has both ends kept
        return gaf

    outs = lambda d: ["-a", d / "o.gaf", "--coverage-out", d / "c.tsv", "--link-coverage-out", d / "l.tsv", "--coverage-gfa-out", d / "g.gfa.gz", "--supported-subgraph-out", d / "s.gfa"]   # noqa: E731
    for name in ("plain", "split", "without"):
        (tmp_path / name).mkdir()
    command("-g", gfa, "-f", fa, "--colinear-gap", GAP, *outs(tmp_path / "plain"))
    gaf = check(tmp_path / "plain")
    command("-g", gfa, "-f", fa, "--colinear-gap", GAP, "--batch-bytes", 3000, "--devices", "0,0", "--inflight", 1, *outs(tmp_path / "split"))      # several batches, two handles merged
    assert check(tmp_path / "split") == gaf
    command("-g", gfa, "-f", fa, "--colinear-gap", GAP, "-a", tmp_path / "without" / "o.gaf")
    assert (tmp_path / "without" / "o.gaf").read_text() == gaf                                                   # the new options leave the alignments alone
    assert sorted(os.listdir(tmp_path / "plain")) == ["c.tsv", "g.gfa.gz", "l.tsv", "o.gaf", "s.gfa"]            # no temporary file stays
