"""The band controls on the device (gc_params::ramp_bandwidth / max_cells_per_slice, the reference's -B / -C): bit-exact against the oracle where
the oracle can judge (a fragment extension is one slice, so the ramp is the wider band there; a limit no slice reaches is no limit), and against
tests/band_model.py through tests/alignment_model.py where only the model can."""
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import seeding_model                                                     # noqa: E402
import test_extension_model as tem                                       # noqa: E402
from alignment_model import AlignmentModel                               # noqa: E402
from band_model import BandModel                                         # noqa: E402
from extension_model import Graph                                        # noqa: E402
from test_gpu_parity import COMPARE_KEYS, compare, expand_stitched_path, gca, mark_missing_chain_alignments, run_case   # noqa: E402,F401
from test_seeding_model import _inputs, std_sort                         # noqa: E402,F401

pytestmark = pytest.mark.gpu

MODEL_LONG_KEYS = ["read_longall_off", "longall_start", "longall_end", "longall_score", "long_trace_off", "long_trace_node", "long_trace_offset", "long_trace_seqpos", "long_trace_switch"]


def device_run(gca, gfa, reads, long_pass, **kw):
    graph = gca.AlignmentGraph(gfa)
    seeder = gca.MinimizerSeeder(graph)
    capacities = kw.pop("capacities", None)
    aligner = gca.Aligner(graph, seeder, keep_traces=True, keep_seeds=True, long_pass=long_pass, chain_traces=2, capacities=capacities, **kw)
    got = {k: (v.astype(np.int64) if v.dtype.kind in "ui" and k not in ("counters", "counters_long") else v) for k, v in aligner.align_reads(reads).items()}
    expand_stitched_path(got, graph.array("nodeLength"))
    mark_missing_chain_alignments(got)
    return got


def band_models(oracle, bandwidth, **band):
    """AlignmentModel over BandModel for the oracle's graph (as tests/test_alignment_model.py builds it over ExtensionModel)."""
    length = oracle.graph_array("nodeLength").tolist()
    flat = oracle.graph_array("sequence")
    seq, at = [], 0
    for n in length:
        seq.append("".join(chr(c) for c in flat[at:at + n]))
        at += n

    def csr(off, adj):
        off, adj = oracle.graph_array(off).tolist(), oracle.graph_array(adj).tolist()
        return [adj[off[i]:off[i + 1]] for i in range(len(length))]
    node_ids, node_offset = oracle.graph_array("nodeIDs").tolist(), oracle.graph_array("nodeOffset").tolist()
    g = Graph(length, seq, csr("out_off", "out_adj"), csr("in_off", "in_adj"), oracle.graph_array("componentNumber").tolist(),
              [bool(x) for x in oracle.graph_array("linearizable")], node_ids, node_offset)
    original_size = {}
    for v, big in enumerate(node_ids):
        original_size[big] = max(original_size.get(big, 0), node_offset[v] + length[v])
    ext = BandModel(g, bandwidth, **band)
    return AlignmentModel(ext, g, original_size), ext


def model_results(gfa, reads, std_sort, bandwidth, whole_read, **band):
    """Per read: the whole-read alignments (start, end, score, trace) and the anchors (x, y, score, path), as the model computes them."""
    from oracle import Oracle
    oracle = Oracle(gfa, long_pass=False)
    graph, index = _inputs(oracle)
    model, ext = band_models(oracle, bandwidth, **band)
    out = []
    for read in reads:
        seeds = seeding_model.order_seeds_by_chaining(seeding_model.get_seeds(read, index, graph, 15, 20, 10.0, std_sort), graph, std_sort)
        alns = []
        if whole_read and seeds:
            got, _ = model.align_one_way(read, seeds, True)
            alns = [(a["start"], a["end"], a["score"], [tuple(c) for c in a["trace"]]) for a in got]
        anchors = [(x, y, score, list(path)) for (x, y, path, first, last, score) in model.anchors_of_read(read, seeding_model.fragment_order(seeds, std_sort))]
        out.append((alns, anchors))
    return out, ext


def device_per_read(got, n):
    out = []
    for r in range(n):
        alns = []
        for a in range(int(got["read_longall_off"][r]), int(got["read_longall_off"][r + 1])) if "read_longall_off" in got and len(got["read_longall_off"]) > r + 1 else []:
            t0, t1 = int(got["long_trace_off"][a]), int(got["long_trace_off"][a + 1])
            trace = list(zip(got["long_trace_node"][t0:t1].tolist(), got["long_trace_offset"][t0:t1].tolist(), got["long_trace_seqpos"][t0:t1].tolist(),
                             [bool(x) for x in got["long_trace_switch"][t0:t1]]))
            alns.append((int(got["longall_start"][a]), int(got["longall_end"][a]), int(got["longall_score"][a]), trace))
        anchors = []
        for b in range(int(got["read_anchor_off"][r]), int(got["read_anchor_off"][r + 1])):
            path = got["anchor_path"][int(got["anchor_path_off"][b]):int(got["anchor_path_off"][b + 1])].tolist()
            anchors.append((int(got["anchor_x"][b]), int(got["anchor_y"][b]), int(got["anchor_score"][b]), path))
        out.append((alns, anchors))
    return out


def assert_model_equal(got, want, reads, whole_read):
    dev = device_per_read(got, len(reads))
    for r in range(len(reads)):
        if got["failed_assertion"][r]:
            continue
        if whole_read:
            assert dev[r][0] == want[r][0], f"read {r}: whole-read alignments differ from the model"
        assert dev[r][1] == want[r][1], f"read {r}: anchors differ from the model"


@pytest.mark.parametrize("slab", [False, True])
@pytest.mark.parametrize("ramp", [16, 30])
def test_fragment_pass_with_the_ramp_is_the_wider_band(gca, tmp_path, monkeypatch, slab, ramp):
    """A fragment extension is one slice: -b 10 -B ramp equals the oracle's -b ramp, anchors, traces, chains, stitched paths and edit distances."""
    from graphchainer_amd.synth import SynthGraph
    if slab:
        monkeypatch.setenv("GC_EXTEND_SLAB", "1")
    sg = SynthGraph(60_000, seed=17, repeats=3)
    gfa = str(tmp_path / "g.gfa")
    sg.write_gfa(gfa)
    reads = sg.sample_reads(24, 2000, seed=5, p_del=0.05, p_sub=0.06, p_ins=0.05)
    _, want = run_case(gca, gfa, reads, long_pass=False, bandwidth=ramp)
    got = device_run(gca, gfa, reads, False, bandwidth=10, ramp_bandwidth=ramp)
    compare(got, want, COMPARE_KEYS)
    assert int(got["read_anchor_off"][-1]) > 100


def _ramp_reads(sg):
    reads = sg.sample_reads(10, 1500, seed=9, p_del=0.07, p_sub=0.08, p_ins=0.07)
    bb = sg.backbone.tobytes()
    rng = random.Random(3)
    reads += [bb[4000:4800] + bb[20000:20800], bb[30000:31200] + bytes(rng.choice(b"ACGT") for _ in range(600))]   # chimeric; leaves the graph
    return reads


@pytest.mark.parametrize("launch", ["default", "reg_cap", "force_fallback", "no_column_store"])
def test_whole_read_pass_with_the_ramp_equals_the_model(gca, tmp_path, monkeypatch, std_sort, launch):
    from graphchainer_amd.synth import SynthGraph
    sg = SynthGraph(40_000, seed=23, repeats=3)
    gfa = str(tmp_path / "g.gfa")
    sg.write_gfa(gfa)
    reads = _ramp_reads(sg)
    kw = {}
    if launch == "reg_cap":
        monkeypatch.setenv("GC_TEST_LONG_REG_CAP", "3")
    elif launch == "force_fallback":
        monkeypatch.setenv("GC_TEST_LONG_FORCE_FALLBACK", "1")
    elif launch == "no_column_store":
        kw["capacities"] = {"long_column_store": -1}
    got = device_run(gca, gfa, reads, True, bandwidth=5, ramp_bandwidth=14, **kw)
    want, ext = model_results(gfa, reads, std_sort, 5, True, ramp_bandwidth=14)
    assert_model_equal(got, want, reads, True)
    assert int(np.sum(got["failed_assertion"])) <= 1
    if launch == "default":   # the rewinds ran in k_long_extend: no read went to the plain-layout fallback, as none does without the ramp
        plain = device_run(gca, gfa, reads, True, bandwidth=5)
        assert int(plain["counters_long"][7]) == 0
        assert int(got["counters_long"][7]) == 0
    assert ext.fired.get("ramp: rewind", 0) > 0
    assert sum(len(alns) for alns, _ in want) >= len(reads)


def _tangle_case(tmp_path):
    rng = random.Random(77)
    (tmp_path / "tangle.gfa").write_text(tem.tangle_gfa(rng, 600))
    gfa = str(tmp_path / "tangle.gfa")
    from oracle import Oracle
    oracle = Oracle(gfa, long_pass=False)
    length = oracle.graph_array("nodeLength").tolist()
    flat = oracle.graph_array("sequence")
    seq, at = [], 0
    for n in length:
        seq.append("".join(chr(c) for c in flat[at:at + n]))
        at += n
    off, adj = oracle.graph_array("out_off").tolist(), oracle.graph_array("out_adj").tolist()
    out = [adj[off[i]:off[i + 1]] for i in range(len(length))]
    comp = oracle.graph_array("componentNumber").tolist()
    first = min(range(len(length)), key=lambda v: comp[v])
    reads = []
    for k in range(12):
        node, text = first, []
        while out[node] and rng.random() < 0.995:
            node = rng.choice(out[node])
            text.append(seq[node])
        text = "".join(text)
        start = rng.randrange(0, max(1, len(text) - 900))
        reads.append(tem.mutate(rng, text[start:start + 800], 0.08).encode())
    return gfa, reads


@pytest.mark.parametrize("whole_read", [False, True])
def test_cell_limit_on_a_tangle_equals_the_model(gca, tmp_path, std_sort, whole_read):
    gfa, reads = _tangle_case(tmp_path)
    limit = 300
    got = device_run(gca, gfa, reads, whole_read, bandwidth=10, max_cells_per_slice=limit)
    want, ext = model_results(gfa, reads, std_sort, 10, whole_read, max_cells_per_slice=limit)
    assert_model_equal(got, want, reads, whole_read)
    assert int(np.sum(got["failed_assertion"])) <= len(reads) // 4
    assert ext.fired.get("cells: break", 0) > 0
    if whole_read:   # (the fragments' one-slice backtraces on this graph pick the same cells with the flag as without)
        assert ext.fired.get("cells: scores not valid", 0) > 0


def test_cell_limit_above_every_slice_is_no_limit(gca, tmp_path, std_sort):
    gfa, reads = _tangle_case(tmp_path)
    _, ext = model_results(gfa, reads, std_sort, 10, True)
    limit = max(ext.slice_cells) + 1
    got, want = run_case(gca, gfa, reads, long_pass=True)
    limited = device_run(gca, gfa, reads, True, bandwidth=10, max_cells_per_slice=limit)
    compare(limited, want, COMPARE_KEYS + MODEL_LONG_KEYS)
    compare(got, want, COMPARE_KEYS + MODEL_LONG_KEYS)


def test_band_controls_are_validated(gca, tmp_path):
    from graphchainer_amd.synth import SynthGraph
    sg = SynthGraph(20_000, seed=3)
    gfa = str(tmp_path / "g.gfa")
    sg.write_gfa(gfa)
    reads = sg.sample_reads(2, 500, seed=1)
    graph = gca.AlignmentGraph(gfa)
    seeder = gca.MinimizerSeeder(graph)
    for kw in ({"bandwidth": 10, "ramp_bandwidth": 10}, {"bandwidth": 10, "ramp_bandwidth": 5}, {"max_cells_per_slice": -2}):
        with pytest.raises(RuntimeError, match="error -1"):
            gca.Aligner(graph, seeder, **kw).align_reads(reads)
    gca.Aligner(graph, seeder, bandwidth=10, ramp_bandwidth=11, max_cells_per_slice=0).align_reads(reads)
