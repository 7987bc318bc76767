"""Precise clipping and the X-drop on the device (gc_params_ext::precise_clipping / x_drop, the reference's --precise-clipping / --X-drop): both extension passes
against tests/precise_model.py through tests/alignment_model.py - the oracle has no such option -, combined with the other extension controls, the stages behind
the extensions by their own properties, the column maximum's arithmetic through its test entry, and the block switched off against the oracle."""
import gzip
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import graphaligner_model as gm                                          # noqa: E402
import seeding_model                                                     # noqa: E402
from alignment_model import AlignmentModel                               # noqa: E402
from extension_model import Graph, ModelAssertion, W                     # noqa: E402
from precise_model import PreciseModel, error_cost, max_x_score_words    # noqa: E402
from test_band_controls_gpu import assert_model_equal, device_per_read, device_run   # noqa: E402
from test_global_alignment_gpu import Inputs, _set_launch                # noqa: E402
from test_gpu_parity import COMPARE_KEYS, LONG_KEYS, compare, gca, run_case   # noqa: E402,F401
from test_precise_model import _column_rows, _extra_reads, _fused_pairs  # noqa: E402
from test_seeding_model import _inputs, std_sort                         # noqa: E402,F401

pytestmark = pytest.mark.gpu

LAUNCHES = ["default", "reg_cap", "force_fallback", "no_column_store"]
SETTINGS = [(0.66, 0), (0.7, 0), (0.66, 5), (0.66, 50)]


class ClipInputs(Inputs):
    """Inputs of tests/test_global_alignment_gpu.py plus the model's results per setting, computed once. A read on which the model trips one of the reference's
    assertions has None in place of its results (the device must report failed_assertion for it)."""

    def __init__(self, directory):
        super().__init__(directory)
        self.whole = self.whole + _extra_reads(self)
        self._clip = {}
        self._world = None

    def world(self):
        if self._world is None:
            from oracle import Oracle
            oracle = Oracle(self.gfa, long_pass=False)
            graph, index = _inputs(oracle)
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
            self._world = (graph, index, g, original_size)
        return self._world

    def clip_model(self, std_sort, which, whole_read, bandwidth=10, split=35, **band):   # noqa: F811
        key = (which, whole_read, bandwidth, split, tuple(sorted(band.items())))
        if key not in self._clip:
            graph, index, g, original_size = self.world()
            ext = PreciseModel(g, bandwidth, **band)
            model = AlignmentModel(ext, g, original_size)
            out = []
            for read in getattr(self, which):
                seeds = seeding_model.order_seeds_by_chaining(seeding_model.get_seeds(read, index, graph, 15, 20, 10.0, std_sort), graph, std_sort)
                try:
                    alns = []
                    if whole_read and seeds:
                        got, _ = model.align_one_way(read, seeds, True)
                        alns = [(a["start"], a["end"], a["score"], [tuple(c) for c in a["trace"]]) for a in got]
                    anchors = [(x, y, score, list(path)) for (x, y, path, first, last, score)
                               in model.anchors_of_read(read, seeding_model.fragment_order(seeds, std_sort), split_len=split, split_gap=split)]
                    out.append((alns, anchors))
                except ModelAssertion:
                    out.append(None)
            self._clip[key] = (out, ext)
        return self._clip[key]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    return ClipInputs(tmp_path_factory.mktemp("clip"))


def _assert_equals_model(got, want, reads, whole_read):
    """Alignment start, end, score, every trace cell, the anchors, failed_assertion, and flatten_ties* == 0."""
    dev = device_per_read(got, len(reads))
    print("device (start, end, score):", [[a[:3] for a in alns] for alns, _ in dev], "anchors", [len(a) for _, a in dev])
    print("model  (start, end, score):", [None if w is None else [a[:3] for a in w[0]] for w in want], "anchors", [None if w is None else len(w[1]) for w in want])
    print("failed_assertion", got["failed_assertion"].tolist(), "capacity_exceeded", got["capacity_exceeded"].tolist())
    assert [bool(x) for x in got["failed_assertion"]] == [w is None for w in want]
    assert int(np.sum(got["capacity_exceeded"])) == 0
    assert_model_equal(got, [w if w is not None else ([], []) for w in want], reads, whole_read)
    assert not np.any(got["flatten_ties"]) and not np.any(got["flatten_ties_long"])


@pytest.mark.parametrize("cutoff,x_drop", SETTINGS)
@pytest.mark.parametrize("launch", LAUNCHES)
def test_whole_read_pass_equals_the_model(gca, inputs, monkeypatch, std_sort, launch, cutoff, x_drop):   # noqa: F811
    kw = _set_launch(monkeypatch, launch)
    got = device_run(gca, inputs.gfa, inputs.whole, True, bandwidth=10, precise_clipping=cutoff, x_drop=x_drop, **kw)
    want, ext = inputs.clip_model(std_sort, "whole", True, precise_clipping=cutoff, x_drop=x_drop)
    _assert_equals_model(got, want, inputs.whole, True)
    assert sum(len(w[0]) for w in want if w) >= len(inputs.whole) - 2
    assert ext.fired.get("clip: ends before the read's end", 0) > 0 and ext.fired.get("clip: best slice is not the last", 0) > 0
    if x_drop:
        assert ext.fired.get("xdrop: stop", 0) > 0
    # a build that trims instead of clipping ends elsewhere: the junk-tailed reads' ends differ from the default's
    default, _ = inputs.clip_model(std_sort, "whole", True)
    assert sum([a[:2] for a in want[r][0]] != [a[:2] for a in default[r][0]] for r in range(len(inputs.whole)) if want[r] and default[r]) >= 3


@pytest.mark.parametrize("cutoff,x_drop", SETTINGS)
@pytest.mark.parametrize("launch", LAUNCHES)
def test_fragment_pass_equals_the_model(gca, inputs, monkeypatch, std_sort, launch, cutoff, x_drop):   # noqa: F811
    """64-base fragments (one full slice per pair of extensions), without the whole-read pass."""
    kw = _set_launch(monkeypatch, launch)
    got = device_run(gca, inputs.gfa, inputs.fragments, False, bandwidth=10, precise_clipping=cutoff, x_drop=x_drop, split_len=64, split_gap=64, **kw)
    want, _ = inputs.clip_model(std_sort, "fragments", False, split=64, precise_clipping=cutoff, x_drop=x_drop)
    _assert_equals_model(got, want, inputs.fragments, False)
    assert sum(len(w[1]) for w in want if w) >= 20
    default, _ = inputs.clip_model(std_sort, "fragments", False, split=64)
    assert sum(want[r] is not None and want[r][1] != default[r][1] for r in range(len(inputs.fragments))) >= 2


def test_clipping_with_the_ramp(gca, inputs, std_sort):   # noqa: F811
    got = device_run(gca, inputs.gfa, inputs.whole, True, bandwidth=10, ramp_bandwidth=25, precise_clipping=0.66)
    want, _ = inputs.clip_model(std_sort, "whole", True, ramp_bandwidth=25, precise_clipping=0.66)
    _assert_equals_model(got, want, inputs.whole, True)


def test_clipping_with_a_cell_limit_that_is_reached(gca, inputs, std_sort):   # noqa: F811
    _, unlimited = inputs.clip_model(std_sort, "whole", True, precise_clipping=0.66)
    cells = sorted(unlimited.slice_cells)
    limit = cells[len(cells) // 4]                                        # the lower quartile: three quarters of the slices reach it
    got = device_run(gca, inputs.gfa, inputs.whole, True, bandwidth=10, max_cells_per_slice=limit, precise_clipping=0.66)
    want, ext = inputs.clip_model(std_sort, "whole", True, max_cells_per_slice=limit, precise_clipping=0.66)
    print("limit", limit, {k: v for k, v in ext.fired.items() if k.startswith("cells:")})
    _assert_equals_model(got, want, inputs.whole, True)
    assert any(c >= limit for c in ext.slice_cells)


def test_clipping_with_the_forced_global_alignment(gca, inputs, std_sort):   # noqa: F811
    got = device_run(gca, inputs.gfa, inputs.whole, True, bandwidth=10, force_global=True, precise_clipping=0.66)
    want, ext = inputs.clip_model(std_sort, "whole", True, force_global=True, precise_clipping=0.66)
    _assert_equals_model(got, want, inputs.whole, True)
    assert "stop: not correct-from-correct" not in ext.fired


def _with_long(off):
    sel = np.repeat(off["read_longall_off"][:-1], np.diff(off["read_long_off"])) + off["long_index"]   # (as run_case: the selected alignments are indices into the read's list)
    for key in ("start", "end", "score"):
        off["long_" + key] = off["longall_" + key][sel]
    return off


def _run(aligner, reads, graph):
    from test_gpu_parity import expand_stitched_path, mark_missing_chain_alignments
    got = {k: (v.astype(np.int64) if v.dtype.kind in "ui" and k not in ("counters", "counters_long") else v) for k, v in aligner.align_reads(reads).items()}
    expand_stitched_path(got, graph.array("nodeLength"))
    mark_missing_chain_alignments(got)
    return _with_long(got)


def test_off_means_off(gca, inputs, monkeypatch):   # noqa: F811
    """ext == NULL (gc_align_batch), gc_align_batch_ext with the block at its defaults, and a batch without clipping behind a clipped one on the same stream: the oracle's results."""
    import ctypes
    from graphchainer_amd.api import GcParamsExt
    reads = inputs.whole
    got, want = run_case(gca, inputs.gfa, reads, long_pass=True)
    compare(got, want, COMPARE_KEYS + LONG_KEYS)
    graph = gca.AlignmentGraph(inputs.gfa)
    seeder = gca.MinimizerSeeder(graph)
    aligner = gca.Aligner(graph, seeder, keep_traces=True, keep_seeds=True, long_pass=True, chain_traces=2)
    compare(_run(aligner, reads, graph), want, COMPARE_KEYS + LONG_KEYS)
    lib, calls = aligner.lib, []

    def with_default_block(g, s, st, batch, params, res):          # gc_align_batch's arguments, sent through gc_align_batch_ext with a block at its defaults
        block = GcParamsExt()
        lib.gc_params_ext_default(ctypes.byref(block))
        calls.append((block.struct_size, block.x_drop, block.precise_clipping))
        return lib.gc_align_batch_ext(g, s, st, batch, None, params, ctypes.byref(block), res)
    with monkeypatch.context() as m:
        m.setattr(lib, "gc_align_batch", with_default_block)
        compare(_run(aligner, reads, graph), want, COMPARE_KEYS + LONG_KEYS)
    assert calls == [(16, 0, 0.0)]
    aligner.params_ext.precise_clipping, aligner.params_ext.x_drop = 0.66, 5
    clipped = _run(aligner, reads, graph)
    assert not np.array_equal(clipped["longall_end"], want["longall_end"]) or not np.array_equal(clipped["anchor_score"], want["anchor_score"])
    aligner.params_ext.precise_clipping, aligner.params_ext.x_drop = 0.0, 0
    compare(_run(aligner, reads, graph), want, COMPARE_KEYS + LONG_KEYS)
    assert int(want["read_longall_off"][-1]) >= len(reads) - 1


@pytest.mark.parametrize("device_output", [1, 2, 4])
def test_the_writers_cope_with_clipped_alignments(gca, inputs, device_output):   # noqa: F811
    """The device's encoders (gc_params::device_output) against the host encoders over the same batch's kept traces: GAF, JSON and GAM of alignments that end mid-read."""
    reads = inputs.whole
    names = [f"r{i}" for i in range(len(reads))]
    graph = gca.AlignmentGraph(inputs.gfa)
    seeder = gca.MinimizerSeeder(graph)
    merge = device_output == 2
    formats = ("json", "gam") if device_output == 4 else ("gaf",)          # (1 / 2: the GAF pieces, with = / X or with M; 4: the vg::Path bytes JSON and GAM wrap)
    kw = dict(long_pass=True, chain_traces=1, precise_clipping=0.66, x_drop=50)
    dev = gca.Aligner(graph, seeder, device_output=device_output, **kw).align_reads(reads, gaf_names=names, cigar_match_mismatch_merge=merge, formats=formats)
    host = gca.Aligner(graph, seeder, keep_traces=True, **kw).align_reads(reads, gaf_names=names, cigar_match_mismatch_merge=merge, formats=formats)
    for f in formats:
        if f == "gam":
            assert gzip.decompress(dev[f]) == gzip.decompress(host[f])
        else:
            assert dev[f] == host[f], f
    for key in ("chained_better", "chain_edit_distance", "long_edit_distance", "failed_assertion"):
        assert np.array_equal(np.asarray(dev[key]), np.asarray(host[key])), key
    if "gaf" in formats:
        # every line of a read whose whole-read alignments win: gc_format_gaf_trace on that alignment's own trace, as the host-side result holds it
        lines = {}
        for line in dev["gaf"].split(b"\n")[:-1]:
            lines.setdefault(line.split(b"\t")[0].decode(), []).append(line)
        checked = 0
        for r in range(len(reads)):
            if host["chained_better"][r] or host["failed_assertion"][r]:
                continue
            picked = [int(host["read_longall_off"][r]) + int(i) for i in host["long_index"][int(host["read_long_off"][r]):int(host["read_long_off"][r + 1])]]
            picked.sort(key=lambda a: int(host["longall_start"][a]))
            expect = []
            for a in picked:
                t0, t1 = int(host["long_trace_off"][a]), int(host["long_trace_off"][a + 1])
                expect.append(gca.api.format_gaf_trace(graph, names[r], reads[r], host["long_trace_node"][t0:t1], host["long_trace_offset"][t0:t1], host["long_trace_seqpos"][t0:t1],
                                                       host["long_trace_switch"][t0:t1], merge=merge))
            assert lines.get(names[r], []) == expect, names[r]
            checked += len(expect)
        print("lines checked against the per-trace formatter:", checked)
        assert checked >= 5
        mid_read = sum(int(f[3]) < int(f[1]) for f in (l.split("\t") for l in dev["gaf"].decode().splitlines()))
        print("GAF lines:", dev["gaf"].count(b"\n"), "ending before the read's end:", mid_read)
        assert mid_read >= 2


def _selected(got, r):
    return got["long_index"][int(got["read_long_off"][r]):int(got["read_long_off"][r + 1])].tolist()


def test_the_cut_off_is_the_evalue_models_identity(gca, inputs, std_sort):   # noqa: F811
    """--E-cutoff and GC_SELECT_GREEDY_E under clipping: E-values of an identity of the clipping cut-off (src/Aligner.cpp:474-482), not of 0.7."""
    reads = inputs.whole
    cutoff = 0.9
    want, _ = inputs.clip_model(std_sort, "whole", True, precise_clipping=cutoff)
    graph = gca.AlignmentGraph(inputs.gfa)
    size = int(graph.SizeInBP())
    alns = [(r, a) for r in range(len(reads)) if want[r] for a in want[r][0]]

    def e_of(identity, r, a):
        return float(gca.api.evalue(identity, size, len(reads[r]), a[1] - a[0], a[2])[1])
    clipped = sorted(e_of(cutoff, r, a) for r, a in alns)
    default = sorted(e_of(0.7, r, a) for r, a in alns)
    e_cutoff = clipped[len(clipped) // 2]
    kept = [[i for i, a in enumerate(want[r][0]) if e_of(cutoff, r, a) <= e_cutoff] if want[r] else [] for r in range(len(reads))]
    kept_default = [[i for i, a in enumerate(want[r][0]) if e_of(0.7, r, a) <= e_cutoff] if want[r] else [] for r in range(len(reads))]
    print("E-values at the cut-off's identity", clipped, "at 0.7", default, "kept", kept, "kept by 0.7", kept_default)
    assert kept != kept_default and any(kept)
    for method in (gm.ALL, gm.GREEDY_E):
        got = device_run(gca, inputs.gfa, reads, True, bandwidth=10, colinear_chaining=False, selection_method=method, e_cutoff=e_cutoff, precise_clipping=cutoff)
        model = [gm.select_alignments([a[:3] for a in want[r][0]], method, size, len(reads[r]), e_cutoff, std_sort, gm.EValue(cutoff)) if want[r] else [] for r in range(len(reads))]
        assert [_selected(got, r) for r in range(len(reads))] == model
        if method == gm.ALL:
            assert [sorted(m) for m in model] == kept
    # with chaining: the whole-read alignments the cut-off keeps
    got = device_run(gca, inputs.gfa, reads, True, bandwidth=10, e_cutoff=e_cutoff, precise_clipping=cutoff)
    model = [gm.select_alignments([a[:3] for a in want[r][0]], gm.GREEDY_LENGTH, size, len(reads[r]), e_cutoff, std_sort, gm.EValue(cutoff)) if want[r] else [] for r in range(len(reads))]
    assert [_selected(got, r) for r in range(len(reads))] == model


def test_the_column_maximum_on_the_device(gca, inputs, std_sort):   # noqa: F811
    """gc_test_max_x_score against WordSlice::maxXScoreLocalMinima as tests/precise_model.py restates it: on the columns the model looked at on this file's reads, and on
    columns built so that the best cell is one of the (cells, score) pairs at which a fused multiply-subtract would truncate to another integer."""
    for cutoff in (0.66, 0.7):
        E = error_cost(cutoff)
        _, ext = inputs.clip_model(std_sort, "whole", True, precise_clipping=cutoff)
        columns = sorted(set(ext.columns_seen))[:40_000]
        built = []
        for cells, score in sorted(_fused_pairs(cutoff, 64))[:200]:
            if score >= cells:
                continue
            # `score` rows rising by one, flat up to row cells - 1, rising again behind it: the best cell is row cells - 1
            vp = ((1 << score) - 1) | (((1 << W) - 1) & ~((1 << cells) - 1))
            built.append((vp, 0, score + W - cells))
        assert built
        for cols, cell_counts in ((columns, (W,)), (built, (W,)), (columns[:5000], (1, 17, 50, 63))):
            vp = np.array([c[0] for c in cols], dtype=np.uint64)
            vn = np.array([c[1] for c in cols], dtype=np.uint64)
            end = np.array([c[2] for c in cols], dtype=np.int32)
            for cells in cell_counts:
                got = gca.api.max_x_scores(vp, vn, end, E, cells)
                want = [max_x_score_words(c[0], c[1], _column_rows(*c)[1], E, cells) for c in cols]
                assert got.tolist() == want, (cutoff, cells)
        fused_differs = sum(max_x_score_words(c[0], c[1], _column_rows(*c)[1], E) != int(float(max(
            (r + 1) - v * Fraction(E) for r, v in enumerate(_column_rows(*c)[0])))) for c in built)
        print("cutoff", cutoff, "columns", len(columns), "built", len(built), "of which a fused evaluation would differ on", fused_differs)
        assert fused_differs > 0
