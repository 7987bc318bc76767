"""The whole-read kernel reads the graph through the per-node record (hip/gc_device.hpp: gcNodeRec and the accessors beside it) and the constant address
space. Held to the oracle where a record says something else than "a plain node with a few edges": (a) IUPAC segments next to plain ones, read in both
directions, so that an ambiguous node (letters outside the record, in ambSeq) is a popped node and a push target; (b) the same graph without a code, so that
the highest-numbered node is a plain one (its record is the last: nothing may be read behind it); (c) reads that run off both ends of the graph (nodes of
degree 0); (d) a hub of 260 arms between two backbone nodes, so that the 8-bit out- and in-degree fields are saturated and the ranges' ends come from the
CSR arrays. Small graphs (under 20 kb), at most 12 reads of 250..3000 bases with ONT-like errors."""
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from graphchainer_amd.synth import SynthGraph                                                        # noqa: E402
from letters_inputs import rewrite_gfa                                                               # noqa: E402
from test_gpu_parity import COMPARE_KEYS, LONG_KEYS, _mutate, _revcomp, compare, gca, run_case       # noqa: E402,F401

BACKBONE = 18_000
ERROR_RATE = 0.10
ARMS = 260


def letters_case(directory, iupac):
    """(gfa path, reads): SynthGraph(18 000) with letters_inputs' rewriting (codes in every third long backbone segment when `iupac`, lower case and U either way),
    ten reads of 250..3000 bases on both strands."""
    sg = SynthGraph(BACKBONE, seed=23, repeats=3)
    plain = os.path.join(str(directory), "plain.gfa")
    sg.write_gfa(plain)
    gfa = os.path.join(str(directory), "letters%d.gfa" % iupac)
    placed = rewrite_gfa(sg, plain, gfa, iupac)
    assert bool(placed) == iupac
    reads = sg.sample_reads(4, 3000, seed=31) + sg.sample_reads(3, 1200, seed=32) + sg.sample_reads(3, 250, seed=33)
    return gfa, reads


def ends_case(directory):
    """(gfa path, reads): reads that start before the graph's first base and end behind its last, both strands: the extension reaches a node without
    in-edges / out-edges and the read's remaining slices find an empty band."""
    sg = SynthGraph(BACKBONE, seed=29)
    gfa = os.path.join(str(directory), "ends.gfa")
    sg.write_gfa(gfa)
    rng, nrng = random.Random(41), np.random.default_rng(41)
    junk = lambda n: bytes(rng.choice(b"ACGT") for _ in range(n))   # noqa: E731
    head = sg.haplotype_window(nrng, 0, 1500).tobytes()
    tail = bytes(sg.backbone[BACKBONE - 1500:].tobytes())
    reads = []
    for n_graph, n_junk in ((1500, 300), (700, 150), (250, 80)):
        reads.append(junk(n_junk) + _mutate(rng, head[:n_graph], ERROR_RATE))
        reads.append(_mutate(rng, tail[-n_graph:], ERROR_RATE) + junk(n_junk))
    reads += [_revcomp(r) for r in reads[:4]]
    return gfa, reads


def hub_case(directory):
    """(gfa path, reads): two backbone segments of 1500 bases joined by 260 distinct arms of 4..6 bases. The last split node of the first segment has 260
    out-edges and the first of the second 260 in-edges (and the same on the reverse strand). Reads cross the hub through one arm, both strands."""
    rng = random.Random(53)
    rand = lambda n: bytes(rng.choice(b"ACGT") for _ in range(n))   # noqa: E731
    a, b = rand(1500), rand(1500)
    arms = set()
    while len(arms) < ARMS:
        arms.add(rand(4 + len(arms) % 3))
    arms = sorted(arms)
    rng.shuffle(arms)
    lines = ["S\t1\t%s\n" % a.decode(), "S\t2\t%s\n" % b.decode()]
    for i, arm in enumerate(arms):
        lines.append("S\t%d\t%s\n" % (3 + i, arm.decode()))
    for i in range(len(arms)):
        lines.append("L\t1\t+\t%d\t+\t0M\n" % (3 + i))
        lines.append("L\t%d\t+\t2\t+\t0M\n" % (3 + i))
    gfa = os.path.join(str(directory), "hub.gfa")
    open(gfa, "w").write("".join(lines))
    reads = []
    for k, (left, right) in enumerate(((1200, 1200), (600, 900), (300, 300), (150, 100), (900, 400), (125, 125))):
        hap = a[len(a) - left:] + arms[(37 * k) % ARMS] + b[:right]
        r = _mutate(rng, hap, ERROR_RATE)
        reads.append(_revcomp(r) if k % 2 else r)
    return gfa, reads


def graph_facts(oracle):
    length = oracle.graph_array("nodeLength")
    out_deg, in_deg = np.diff(oracle.graph_array("out_off")), np.diff(oracle.graph_array("in_off"))
    letters = oracle.graph_array("sequence")
    first = np.concatenate([[0], np.cumsum(length)])
    ambiguous = np.array([np.any(~np.isin(letters[first[i]:first[i + 1]], [ord(c) for c in "ACGT"])) for i in range(len(length))])
    return length, out_deg, in_deg, ambiguous


def every_read_aligns(want, n_reads):
    per_read = np.diff(np.asarray(want["read_longall_off"]))
    assert len(per_read) == n_reads and np.all(per_read >= 1), per_read


def test_the_inputs_are_what_they_are_meant_to_be(tmp_path):
    """On the CPU, with the oracle alone: every read of every case has a whole-read alignment, and the graphs hold what the cases are about."""
    from oracle import Oracle
    for iupac in (True, False):
        gfa, reads = letters_case(tmp_path, iupac)
        assert len(reads) <= 12 and all(250 <= len(r) <= 3000 for r in reads)
        o = Oracle(gfa, long_pass=True)
        length, out_deg, in_deg, ambiguous = graph_facts(o)
        assert int(length.sum()) <= 2 * 20_000 and length.min() == 1 and length.max() == 64   # (both strands)
        if iupac:
            # ambiguous nodes with plain in- and out-neighbours: they are popped after a plain node pushed them, and push plain ones
            out_off, out_adj = o.graph_array("out_off"), o.graph_array("out_adj")
            plain_to_amb = sum(1 for v in np.nonzero(~ambiguous)[0] for t in out_adj[out_off[v]:out_off[v + 1]] if ambiguous[t])
            amb_to_plain = sum(1 for v in np.nonzero(ambiguous)[0] for t in out_adj[out_off[v]:out_off[v + 1]] if not ambiguous[t])
            assert ambiguous.sum() > 50 and plain_to_amb > 50 and amb_to_plain > 50
        else:
            assert not ambiguous.any()   # firstAmbiguous == n: the highest-numbered node is a plain one
        every_read_aligns(o.align(reads), len(reads))
    gfa, reads = ends_case(tmp_path)
    assert len(reads) <= 12 and all(250 <= len(r) <= 3000 for r in reads)
    o = Oracle(gfa, long_pass=True)
    length, out_deg, in_deg, ambiguous = graph_facts(o)
    assert (out_deg == 0).sum() >= 2 and (in_deg == 0).sum() >= 2
    every_read_aligns(o.align(reads), len(reads))
    gfa, reads = hub_case(tmp_path)
    assert len(reads) <= 12 and all(250 <= len(r) <= 3000 for r in reads)
    o = Oracle(gfa, long_pass=True)
    length, out_deg, in_deg, ambiguous = graph_facts(o)
    assert int(length.sum()) <= 2 * 20_000
    assert (out_deg == ARMS).sum() == 2 and (in_deg == ARMS).sum() == 2   # one per strand: both degree fields saturate
    every_read_aligns(o.align(reads), len(reads))


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["iupac", "plain", "ends"])
def test_record_reads_against_the_oracle(gca, tmp_path, case):
    gfa, reads = letters_case(tmp_path, True) if case == "iupac" else letters_case(tmp_path, False) if case == "plain" else ends_case(tmp_path)
    got, want = run_case(gca, gfa, reads, long_pass=True)
    every_read_aligns(want, len(reads))
    fallback, column_steps = int(got["counters_long"][7]), int(got["counters_long"][2])
    print(f"{case}: plain-layout reruns {fallback} of {len(reads)} reads, column steps {column_steps}")
    assert fallback == 0, "a read left the one-extension-per-wave kernel"
    assert column_steps > 0
    compare(got, want, COMPARE_KEYS + LONG_KEYS)


@pytest.mark.gpu
def test_saturated_degree_fields_against_the_oracle(gca, tmp_path):
    """The hub, a batch of its own. Its slices hold up to 260 nodes and the band tables 64, so these reads are expected to go on to the retry or to the
    plain-layout kernel - after the one-extension-per-wave kernel has taken the out-edge range's end from outOff[node + 1]."""
    gfa, reads = hub_case(tmp_path)
    got, want = run_case(gca, gfa, reads, long_pass=True)
    every_read_aligns(want, len(reads))
    print(f"hub: plain-layout reruns {int(got['counters_long'][7])} of {len(reads)} reads, column steps {int(got['counters_long'][2])}")
    compare(got, want, COMPARE_KEYS + LONG_KEYS)
