"""gc_params::fast_mode (the reference's --fast-mode, src/Aligner.cpp:834-843) on the device against tests/fastmode_model.py - the oracle has no such option.
The model is fed from a fast_mode=False run of the same batch, which is itself held to the oracle; every array the flag does not touch must be equal in the two runs."""
import gzip
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from fastmode_model import fast_chained_alignment, path_to_trace          # noqa: E402
from test_gpu_parity import COMPARE_KEYS, LONG_KEYS, compare, gca, run_case   # noqa: E402,F401

pytestmark = pytest.mark.gpu

GAP = 200   # --colinear-gap of every run here: the chimera's chain is split at its jump of a few thousand bases
TRACE_KEYS = ["read_chain_trace_off", "chain_trace_node", "chain_trace_offset", "chain_trace_seqpos", "chain_trace_switch", "chain_aln_start", "chain_aln_end"]
# what the flag must leave alone (long_pass=False runs have empty long_* arrays, which are compared all the same)
UNTOUCHED = ["read_seed_off", "seed_node", "seed_offset", "seed_seqpos", "seed_goodness", "read_anchor_off", "anchor_x", "anchor_y", "anchor_path_off", "anchor_path",
             "anchor_first_node", "anchor_first_offset", "anchor_first_seqpos", "anchor_last_node", "anchor_last_offset", "anchor_last_seqpos", "anchor_score",
             "read_chain_off", "chain", "chain_score", "failed_assertion", "capacity_exceeded", "seeds_extended", "flatten_ties", "read_path_off", "path_node",
             "path_first_offset", "path_last_offset", "path_cells", "read_longall_off", "longall_start", "longall_end", "longall_score", "read_long_off", "long_index",
             "long_edit_distance", "seeds_extended_long", "flatten_ties_long"]


def make_reads(sg):
    """(reads, index of the one-node read, of the chimera, of the random read)"""
    bb = sg.backbone.tobytes()
    rng = np.random.default_rng(41)

    def substituted(a, n, every):
        s = bytearray(bb[a:a + n])
        for i in range(every // 2, n, every):
            s[i] = b"ACGT"[(b"ACGT".index(s[i]) + 1) % 4]
        return bytes(s)

    # a backbone segment of 48 bases or more is one split node over its first 48: 35 bases cut from inside it
    seg = next(i for i in range(len(sg.seg_start)) if sg.seg_start[i] > 9000 and sg.seg_end[i] - sg.seg_start[i] >= 48)
    one_node = bb[int(sg.seg_start[seg]) + 4:int(sg.seg_start[seg]) + 39]
    reads = sg.sample_reads(2, 500, seed=5, p_del=0.0, p_sub=0.06, p_ins=0.0)          # substitutions only
    reads += sg.sample_reads(3, 600, seed=6)                                             # the default indel mix
    reads += sg.sample_reads(1, 400, seed=7, p_del=0.0, p_sub=0.02, p_ins=0.10)         # read longer than its path ...
    reads += sg.sample_reads(1, 400, seed=8, p_del=0.10, p_sub=0.02, p_ins=0.0)         # ... and shorter
    i_one = len(reads)
    reads.append(one_node)
    reads += [bb[14000:14036], bb[15000:15064], bb[16000:16065], bb[17000:17070]]        # reads around 64 bases: one or two 35-base fragments, a piece of 35 to 70 cells
    reads += [bb[14000:14035] + bb[14000 + k:14035 + k] for k in (28, 29, 30)]          # two fragments that overlap on the graph: pieces of 63, 64 and 65 cells
    reads.append(substituted(21000, 4300, 211))                                          # more than 64 path nodes
    i_chimera = len(reads)
    reads.append(bb[5000:5400] + bb[8200:8800])
    # a backbone read carrying a block of junk the whole-read pass cannot cross
    reads.append(bb[31000:31300] + bytes(rng.choice(list(b"ACGT"), size=250).tolist()) + bb[31300:31700])
    i_random = len(reads)
    reads.append(bytes(rng.choice(list(b"ACGT"), size=500).tolist()))
    return reads, i_one, i_chimera, i_random


class World:
    """The graph, the reads and the fast_mode=False runs that everything here is compared with, made once."""

    def __init__(self, gca, directory):
        from graphchainer_amd.synth import SynthGraph
        self.gca = gca
        self.sg = SynthGraph(40_000, seed=23, repeats=3)
        self.gfa = os.path.join(str(directory), "g.gfa")
        self.sg.write_gfa(self.gfa)
        self.reads, self.i_one, self.i_chimera, self.i_random = make_reads(self.sg)
        self.names = [f"r{i}" for i in range(len(self.reads))]
        self.graph = gca.AlignmentGraph(self.gfa)
        self.seeder = gca.MinimizerSeeder(self.graph)
        self.node_length = self.graph.array("nodeLength")
        self.node_ids = self.graph.array("nodeIDs")
        self.node_offset = self.graph.array("nodeOffset")
        self.bp = int(np.sum(self.node_length))
        # the default mode, against the oracle (as test_off_means_off of the forced global alignment does)
        self.base, want = run_case(gca, self.gfa, self.reads, long_pass=False, colinear_gap=GAP)
        compare(self.base, want, COMPARE_KEYS)
        self.base_long, want_long = run_case(gca, self.gfa, self.reads, long_pass=True, colinear_gap=GAP)
        compare(self.base_long, want_long, COMPARE_KEYS + LONG_KEYS)
        self.model = self.models(self.base)
        self.model_long = self.models(self.base_long)

    def align(self, reads=None, aligner=None, **kw):
        aligner = aligner or self.aligner(**kw)
        return {k: (np.asarray(v).astype(np.int64) if isinstance(v, np.ndarray) and v.dtype.kind in "ui" else v) for k, v in aligner.align_reads(self.reads if reads is None else reads).items()}

    def aligner(self, **kw):
        kw.setdefault("colinear_gap", GAP)
        return self.gca.Aligner(self.graph, self.seeder, **kw)

    def models(self, got, reads=None):
        """Per read the model's (node, offset, seqpos, switch, score, start, end), or None for a read without a stitched piece. `got`: a fast_mode=False result as
        run_case returns it (path_nodes_raw: the stitched piece's node list)."""
        reads = self.reads if reads is None else reads
        out = []
        off, raw = raw_path_off(got), got["path_nodes_raw"]
        assert int(off[-1]) == len(raw)
        for r, read in enumerate(reads):
            path = [int(v) for v in raw[off[r]:off[r + 1]]]
            chain = got["chain"][got["read_chain_off"][r]:got["read_chain_off"][r + 1]]
            if not path or not len(chain) or got["failed_assertion"][r]:
                out.append(None)
                continue
            a0 = int(got["read_anchor_off"][r])
            x, y = int(got["anchor_x"][a0 + chain[0]]), int(got["anchor_y"][a0 + chain[-1]])
            first, last = int(got["path_first_offset"][r]), int(got["path_last_offset"][r])
            cells = path_to_trace(path, first, last, self.node_length)
            assert len(cells) == int(got["path_cells"][r])
            text = self.gca.api.graph_letters(self.graph, [self.node_ids[v] for v, _ in cells], [o + self.node_offset[v] for v, o in cells])
            letters = {cell: chr(c) for cell, c in zip(cells, text)}
            out.append(fast_chained_alignment(path, first, last, x, y, read, self.node_length, self.node_ids, self.node_offset, lambda v, o: letters[(v, o)]))
        return out


@pytest.fixture(scope="module")
def world(gca, tmp_path_factory):
    return World(gca, tmp_path_factory.mktemp("fastmode"))


def per_read_trace(got, r):
    a, b = int(got["read_chain_trace_off"][r]), int(got["read_chain_trace_off"][r + 1])
    return [got[k][a:b].tolist() for k in ("chain_trace_node", "chain_trace_offset", "chain_trace_seqpos", "chain_trace_switch")]


def assert_untouched(fast, base):
    for key in UNTOUCHED:
        assert np.array_equal(np.asarray(fast[key]), np.asarray(base[key])), key


def assert_traces_equal_the_model(got, model, traced):
    for r, m in enumerate(model):
        if m is None or not traced[r]:
            assert per_read_trace(got, r) == [[], [], [], []], r
            assert (int(got["chain_aln_start"][r]), int(got["chain_aln_end"][r])) == (0, 0), r
            continue
        assert per_read_trace(got, r) == [list(m[0]), list(m[1]), list(m[2]), list(m[3])], f"read {r}"
        assert (int(got["chain_aln_start"][r]), int(got["chain_aln_end"][r])) == (m[5], m[6]), r


def raw_path_off(base):
    """read_path_off of the stitched pieces' NODE lists (run_case leaves read_path_off per cell)."""
    return np.concatenate([[0], np.cumsum([len(set(base["path_node"][a:b].tolist())) for a, b in zip(base["read_path_off"][:-1], base["read_path_off"][1:])])])


def test_the_inputs_hold_the_cases(world):
    """The conditions the reads were chosen for, from the default run's arrays (the same that the oracle gave when the reads were chosen)."""
    base, model = world.base, world.model
    off = raw_path_off(base)
    n_nodes = np.diff(off)
    cells = base["path_cells"]
    spans = {}
    for r, m in enumerate(model):
        if m is None:
            continue
        chain = base["chain"][base["read_chain_off"][r]:base["read_chain_off"][r + 1]]
        a0 = int(base["read_anchor_off"][r])
        spans[r] = (int(base["anchor_x"][a0 + chain[0]]), int(base["anchor_y"][a0 + chain[-1]]), int(cells[r]))
    print("path nodes", n_nodes.tolist(), "cells", cells.tolist(), "(x, y, n)", spans)
    assert model[world.i_random] is None and len(spans) >= len(world.reads) - 2          # the random read has no chain; all but one of the others have a stitched piece
    assert n_nodes[world.i_one] == 1                                                        # a one-node piece
    assert any(n > y - x + 1 for x, y, n in spans.values())                                # the clamp repeats y
    assert any(n < y - x + 1 for x, y, n in spans.values())                                # the trace ends before y
    assert n_nodes.max() > 64                                                               # the scan's second turn
    assert {63, 64, 65} <= {int(c) for c in cells}                                          # cell counts around one turn of 64 lanes
    # the x quirk: the chimera's chain is split and the later piece is the longest - its first node is not on the chain's first anchor
    r = world.i_chimera
    chain = base["chain"][base["read_chain_off"][r]:base["read_chain_off"][r + 1]]
    a = int(base["read_anchor_off"][r]) + int(chain[0])
    first_anchor_nodes = set(base["anchor_path"][base["anchor_path_off"][a]:base["anchor_path_off"][a + 1]].tolist())
    assert int(world.base["path_nodes_raw"][off[r]]) not in first_anchor_nodes
    assert spans[r][0] < 100 and model[r][2][0] == spans[r][0]                              # ... and the trace still starts at the chain's x


def test_fast_mode_equals_the_model(world):
    """long_pass=False: every read with a stitched piece wins, so every one is traced (chain_traces=1)."""
    got = world.align(fast_mode=True, long_pass=False, chain_traces=1, keep_seeds=True)
    base = world.align(fast_mode=False, long_pass=False, chain_traces=1, keep_seeds=True)
    assert_untouched(got, base)
    model = world.model
    stitched = [m is not None for m in model]
    print("scores", [m[4] if m else None for m in model], "default mode's NW distances", base["chain_edit_distance"].tolist())
    assert got["chain_edit_distance"].tolist() == [m[4] if m else -1 for m in model]
    assert got["chained_better"].tolist() == [int(s) for s in stitched]
    assert_traces_equal_the_model(got, model, stitched)
    assert np.array_equal(np.diff(got["read_chain_trace_off"]), np.where(stitched, got["path_cells"], 0))   # one cell per path base
    assert not np.any(got["capacity_exceeded"])


def test_the_decision_with_the_whole_read_pass(world):
    got = world.align(fast_mode=True, long_pass=True, chain_traces=2, keep_seeds=True)
    base = world.align(fast_mode=False, long_pass=True, chain_traces=2, keep_seeds=True)
    assert_untouched(got, base)
    model = world.model_long
    stitched = [m is not None for m in model]
    assert_traces_equal_the_model(got, model, stitched)                                     # traces for every stitched read, winner or not
    selected = np.diff(got["read_long_off"]) > 0
    want = [int(m is not None and (not selected[r] or int(got["long_edit_distance"][r]) > m[4])) for r, m in enumerate(model)]
    print("scores", [m[4] if m else None for m in model], "long_edit_distance", got["long_edit_distance"].tolist(), "chained_better", want)
    assert got["chain_edit_distance"].tolist() == [m[4] if m else -1 for m in model]
    assert got["chained_better"].tolist() == want
    assert 0 < sum(want) < sum(stitched)                                                    # at least one read wins, at least one loses


def test_trace_modes_and_the_e_cutoff(world):
    model = world.model_long
    full = world.align(fast_mode=True, long_pass=True, chain_traces=2)
    winners = full["chained_better"].astype(bool).tolist()
    one = world.align(fast_mode=True, long_pass=True, chain_traces=1)
    assert one["chained_better"].tolist() == full["chained_better"].tolist()
    assert_traces_equal_the_model(one, model, winners)                                      # the winners only
    none = world.align(fast_mode=True, long_pass=True, chain_traces=0)
    assert none["chained_better"].tolist() == full["chained_better"].tolist()
    assert none["chain_edit_distance"].tolist() == full["chain_edit_distance"].tolist()
    assert int(none["read_chain_trace_off"][-1]) == 0
    # --E-cutoff (:904) sees the fast alignment's own bounds and score: a cut-off between two reads' E-values drops exactly the reads above it
    model = world.model
    evalues = {r: float(world.gca.api.evalue(0.7, world.bp, len(world.reads[r]), m[6] - m[5], m[4])[1]) for r, m in enumerate(model) if m is not None}
    ordered = sorted(set(evalues.values()))
    print("E-values", evalues)
    assert len(ordered) >= 2
    cut = (ordered[len(ordered) // 2 - 1] + ordered[len(ordered) // 2]) / 2
    kept = [m is not None and evalues[r] <= cut for r, m in enumerate(model)]
    assert any(kept) and any(m is not None and not k for m, k in zip(model, kept))
    got = world.align(fast_mode=True, long_pass=False, chain_traces=2, e_cutoff=cut)
    assert got["chained_better"].tolist() == [int(k) for k in kept]
    assert_traces_equal_the_model(got, model, kept)


@pytest.mark.parametrize("merge", [False, True])
def test_output(world, merge):
    gca, names = world.gca, world.names
    dev = world.aligner(fast_mode=True, long_pass=True, chain_traces=1, device_output=(2 if merge else 1) | 4).align_reads(
        world.reads, gaf_names=names, cigar_match_mismatch_merge=merge, other_formats=True)
    host = world.aligner(fast_mode=True, long_pass=True, chain_traces=1, keep_traces=True).align_reads(
        world.reads, gaf_names=names, cigar_match_mismatch_merge=merge, other_formats=True)
    assert dev["gaf"] == host["gaf"]
    assert dev["gaf_chained_skipped"] == 0 and host["gaf_chained_skipped"] == 0
    winners = [r for r in range(len(names)) if dev["chained_better"][r]]
    assert winners and int(np.sum(dev["out_source"])) == len(winners)
    lines = {}
    for line in dev["gaf"].split(b"\n"):
        if line:
            lines.setdefault(line.split(b"\t")[0].decode(), []).append(line)
    ended_early = 0
    for r in winners:
        m = world.model_long[r]
        assert lines[names[r]] == [gca.api.format_gaf_trace(world.graph, names[r], world.reads[r], m[0], m[1], m[2], m[3], merge=merge)], names[r]
        ended_early += m[2][-1] + 1 < len(world.reads[r])                                   # a trace that ends before the read does
    assert ended_early >= 1
    # without the whole-read pass every stitched read is written from its chained alignment, the ones whose read position repeats at the clamp y among them
    every = world.aligner(fast_mode=True, long_pass=False, chain_traces=1, keep_traces=True).align_reads(world.reads, gaf_names=names, cigar_match_mismatch_merge=merge)
    assert every["gaf_chained_skipped"] == 0
    want, clamped = [], 0
    for r, m in enumerate(world.model):
        if m is not None:
            want.append(gca.api.format_gaf_trace(world.graph, names[r], world.reads[r], m[0], m[1], m[2], m[3], merge=merge))
            clamped += len(m[2]) >= 2 and m[2][-1] == m[2][-2]
    assert every["gaf"].split(b"\n")[:-1] == want
    print("winners", winners, "ending before the read's end", ended_early, "reads with a repeated last position", clamped)
    assert clamped >= 1
    # JSON lines and GAM: the two routes agree, both decode, and a winner's message carries the path of its GAF line
    assert dev["json"] == host["json"]
    assert gzip.decompress(dev["gam"]) == gzip.decompress(host["gam"])
    objects = {}
    for text in dev["json"].decode().splitlines():
        o = json.loads(text)
        objects.setdefault(o["name"], []).append(o)
    for r in winners:
        (o,) = objects[names[r]]
        steps = [(">" if not m["position"].get("is_reverse") else "<") + str(m["position"].get("name", m["position"].get("node_id"))) for m in o["path"]["mapping"]]
        assert "".join(steps).encode() == lines[names[r]][0].split(b"\t")[5], names[r]


@pytest.mark.parametrize("env, on_host", [({"GC_HOST_STITCH": "1"}, "all"), ({"GC_TEST_STITCH_SET_MAX": "20"}, "some")])
def test_pieces_stitched_on_the_host(world, monkeypatch, env, on_host):
    """The kernels read a piece's nodes where the stitching left them: in the stitching kernel's output, or in the list the host uploads for the reads it stitched itself."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got = world.align(fast_mode=True, long_pass=False, chain_traces=1)
    stitched = [m is not None for m in world.model]
    print("reads stitched on the host:", int(got["counters"][7]), "of", sum(stitched))
    assert int(got["counters"][7]) == sum(stitched) if on_host == "all" else 0 < int(got["counters"][7]) < sum(stitched)
    assert got["chain_edit_distance"].tolist() == [m[4] if m else -1 for m in world.model]
    assert_traces_equal_the_model(got, world.model, stitched)


def test_launch_shapes(world):
    """One read alone; the whole list twice on one stream (the second batch finds the stream's pools as the first left them)."""
    r = world.i_chimera
    alone = world.align(reads=[world.reads[r]], fast_mode=True, long_pass=False, chain_traces=1)
    m = world.model[r]
    assert per_read_trace(alone, 0) == [list(m[0]), list(m[1]), list(m[2]), list(m[3])]
    assert int(alone["chain_edit_distance"][0]) == m[4]
    aligner = world.aligner(fast_mode=True, long_pass=True, chain_traces=2)
    first = world.align(aligner=aligner)
    second = world.align(aligner=aligner)
    for key in UNTOUCHED + TRACE_KEYS + ["chain_edit_distance", "chained_better"]:
        assert np.array_equal(first[key], second[key]), key
    assert_traces_equal_the_model(second, world.model_long, [m is not None for m in world.model_long])


def test_argument_checks(world):
    with pytest.raises(RuntimeError, match="error -1"):
        world.aligner(fast_mode=2).align_reads(world.reads[:2])
    # without chaining the flag is accepted and never looked at (src/Aligner.cpp:596-600)
    plain = world.align(long_pass=True, colinear_chaining=False)
    flagged = world.align(long_pass=True, colinear_chaining=False, fast_mode=True)
    for key in UNTOUCHED + TRACE_KEYS + ["chain_edit_distance", "chained_better"]:
        assert np.array_equal(plain[key], flagged[key]), key
