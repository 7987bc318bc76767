"""The seed-extension heuristics and the mode without chaining on the device (gc_params::seed_extend_density / extra_heuristic / colinear_chaining / selection_method,
the reference's --seeds-extend-density / --extra-heuristic / --no-colinear-chaining and its selection methods). The oracle has none of them, so the yardstick is
tests/graphaligner_model.py; with all four at their defaults the oracle judges. The inputs are those of tests/test_graphaligner_model.py, which shows on the CPU that
the rules have something to cut on them."""
import gzip
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import graphaligner_model as gm                                           # noqa: E402
from corrected_model import output_order                                  # noqa: E402
from test_band_controls_gpu import assert_model_equal, device_per_read, device_run   # noqa: E402
from test_gpu_parity import COMPARE_KEYS, LONG_KEYS, compare, expand_stitched_path, gca, mark_missing_chain_alignments, run_case   # noqa: E402,F401
from test_graphaligner_model import DENSITIES, as_hit, inputs             # noqa: E402,F401  (the module's inputs, built once)
from test_seeding_model import std_sort                                   # noqa: E402,F401
from vg_descriptor import decode_gam_stream                               # noqa: E402

pytestmark = pytest.mark.gpu

LAUNCHES = ["default", "reg_cap", "force_fallback"]
EMPTY = ["anchor_x", "anchor_y", "anchor_path", "anchor_score", "chain", "path_node", "chain_trace_node", "chain_trace_offset", "chain_trace_seqpos", "chain_trace_switch"]
ZERO_OFFSETS = ["read_anchor_off", "read_chain_off", "read_path_off", "read_chain_trace_off"]


def _set_launch(monkeypatch, launch, speculate):
    if launch == "reg_cap":
        monkeypatch.setenv("GC_TEST_LONG_REG_CAP", "3")
    elif launch == "force_fallback":
        monkeypatch.setenv("GC_TEST_LONG_FORCE_FALLBACK", "1")
    if speculate is not None:
        monkeypatch.setenv("GC_TEST_LONG_SPECULATE", speculate)     # 1: one seed per round in every round; 2: two candidates from round 0 on


def _seeded_run(gca, inputs, **kw):   # noqa: F811
    """The seeded reads with their caller-supplied hits through gc_align_batch_seeded, normalised as device_run does."""
    graph = gca.AlignmentGraph(inputs.gfa)
    batch = gca.ReadBatch(inputs.seeded_reads)
    seeds = gca.SeedBatch(graph, batch, [[as_hit(s) for s in hits] for hits in inputs.seeded_hits])
    out = gca.Aligner(graph, None, keep_traces=True, keep_seeds=True, long_pass=True, chain_traces=2, **kw).align_batch(batch, seeds=seeds)
    got = {k: (v.astype(np.int64) if v.dtype.kind in "ui" and k not in ("counters", "counters_long") else v) for k, v in out.items()}
    expand_stitched_path(got, graph.array("nodeLength"))
    mark_missing_chain_alignments(got)
    return got


def _assert_equals_model(got, want, reads):
    """longall_*, every trace cell and seeds_extended_long against the model's (alignments, seeds extended) per read; no anchors without chaining."""
    print("device (start, end, score):", [[a[:3] for a in alns] for alns, _ in device_per_read(got, len(reads))], "seeds extended", got["seeds_extended_long"].tolist())
    print("model  (start, end, score):", [[a[:3] for a in alns] for alns, _ in want], "seeds extended", [x[1] for x in want])
    assert not np.any(got["failed_assertion"]) and not np.any(got["capacity_exceeded"])
    assert_model_equal(got, [(alns, []) for alns, _ in want], reads, True)
    assert got["seeds_extended_long"].tolist() == [x[1] for x in want]


def _assert_nothing_chained(got, n):
    for key in EMPTY:
        assert len(got[key]) == 0, key
    for key in ZERO_OFFSETS:
        assert got[key].tolist() == [0] * (n + 1), key
    assert got["anchor_path_off"].tolist() == [0]
    assert got["chained_better"].tolist() == [0] * n
    assert got["long_edit_distance"].tolist() == [-1] * n and got["chain_edit_distance"].tolist() == [-1] * n
    assert got["seeds_extended"].tolist() == [0] * n and got["chain_score"].tolist() == [0] * n


@pytest.mark.parametrize("speculate", ["1", "2"])
@pytest.mark.parametrize("launch", LAUNCHES)
def test_seed_budget_equals_the_model(gca, inputs, monkeypatch, launch, speculate):   # noqa: F811
    """Three densities: extendSeeds is 1 for every read, 1 or 2, and 1 to 4 by the read's length (DENSITIES). The chimeras lose their later alignments, the junk-tailed
    read whose second seed is as good as its first keeps both (the tie rule of :132)."""
    _set_launch(monkeypatch, launch, speculate)
    for density in DENSITIES:
        got = device_run(gca, inputs.gfa, inputs.reads, True, bandwidth=10, colinear_chaining=False, selection_method=gm.ALL, seed_extend_density=density)
        _assert_equals_model(got, inputs.run(False, density), inputs.reads)
        _assert_nothing_chained(got, len(inputs.reads))
        if launch == "default":
            assert int(got["counters_long"][7]) == 0
    cut = inputs.run(False, DENSITIES[0])
    assert sum(len(cut[r][0]) < len(inputs.run(False)[r][0]) for r in range(len(inputs.reads))) >= 3


def test_seed_budget_with_the_tail_rounds_own_speculation(gca, inputs):   # noqa: F811
    """No test hook: a batch this small tries up to eight seeds per read from the second round on."""
    for density in DENSITIES[:2]:
        got = device_run(gca, inputs.gfa, inputs.reads, True, bandwidth=10, colinear_chaining=False, seed_extend_density=density)
        _assert_equals_model(got, inputs.run(False, density), inputs.reads)


@pytest.mark.parametrize("speculate", ["1", "2"])
@pytest.mark.parametrize("launch", LAUNCHES)
def test_extra_heuristic_equals_the_model(gca, inputs, monkeypatch, launch, speculate):   # noqa: F811
    """On and off, on the seeded reads (two clusters of one goodness: off extends the second copy's seeds, on stops at :127 or skips them at :152) and on the
    minimizer-seeded reads; with a seed budget of 1 the flag ends the scan whatever the next seed's goodness (:132).
    No read here has a best seed of goodness 0, and the seed order cannot produce one: orderSeedsByChaining gives every seed its cluster's matching bases plus
    its raw goodness, a cluster's first seed contributes matchLen - 1 bases, and the reference asserts matchLen >= 2 (src/GraphAligner.h:280). So goodness >= 1."""
    _set_launch(monkeypatch, launch, speculate)
    for flag in (False, True):
        got = _seeded_run(gca, inputs, colinear_chaining=False, extra_heuristic=flag)
        _assert_equals_model(got, inputs.run(True, -1, flag), inputs.seeded_reads)
        got = device_run(gca, inputs.gfa, inputs.reads, True, bandwidth=10, colinear_chaining=False, extra_heuristic=flag)
        _assert_equals_model(got, inputs.run(False, -1, flag), inputs.reads)
    for flag in (False, True):
        got = _seeded_run(gca, inputs, colinear_chaining=False, extra_heuristic=flag, seed_extend_density=DENSITIES[0])
        _assert_equals_model(got, inputs.run(True, DENSITIES[0], flag), inputs.seeded_reads)
    off, on = inputs.run(True), inputs.run(True, -1, True)
    assert sum(off[r][1] != on[r][1] for r in range(len(inputs.seeded_reads))) >= 2


def test_extra_heuristic_leaves_the_fragment_pass_alone(gca, inputs):   # noqa: F811
    """With chaining on the flag reaches the whole-read pass only: anchors, chains and stitched paths are those of the run without it."""
    off = device_run(gca, inputs.gfa, inputs.reads, True, bandwidth=10)
    on = device_run(gca, inputs.gfa, inputs.reads, True, bandwidth=10, extra_heuristic=True)
    for key in ("read_anchor_off", "anchor_x", "anchor_y", "anchor_score", "anchor_path", "read_chain_off", "chain", "chain_score", "path_node", "seeds_extended", "chain_edit_distance"):
        assert np.array_equal(off[key], on[key]), key
    assert int(off["read_anchor_off"][-1]) > 100
    want = inputs.run(False, -1, True)
    assert on["seeds_extended_long"].tolist() == [x[1] for x in want]


def test_defaults_equal_the_oracle(gca, inputs):   # noqa: F811
    got, want = run_case(gca, inputs.gfa, inputs.reads, long_pass=True)
    compare(got, want, COMPARE_KEYS + LONG_KEYS)
    spelled = device_run(gca, inputs.gfa, inputs.reads, True, bandwidth=10, seed_extend_density=-1.0, extra_heuristic=False, colinear_chaining=True, selection_method=0)
    sel = np.repeat(spelled["read_longall_off"][:-1], np.diff(spelled["read_long_off"])) + spelled["long_index"]
    for key in ("start", "end", "score"):
        spelled["long_" + key] = spelled["longall_" + key][sel]
    compare(spelled, want, COMPARE_KEYS + LONG_KEYS)
    assert int(want["read_longall_off"][-1]) >= len(inputs.reads) + 4


def _selected(got, r):
    return got["long_index"][int(got["read_long_off"][r]):int(got["read_long_off"][r + 1])].tolist()


@pytest.mark.parametrize("method", range(8))
def test_without_chaining_selection_equals_the_model(gca, inputs, method):   # noqa: F811
    """read_long_off / long_index are SelectAlignments(method) of the read's list, in the order it returns them - without a cut-off and with one that drops the
    shorter alignments - and nothing of the chaining side comes back."""
    model = inputs.run(False)
    ev = gm.EValue()
    evalues = sorted(ev.evalue(inputs.graph_size, len(inputs.reads[r]), a[1] - a[0], a[2]) for r in range(len(inputs.reads)) for a in model[r][0])
    for e_cutoff in (-1.0, evalues[len(evalues) // 2]):
        got = device_run(gca, inputs.gfa, inputs.reads, True, bandwidth=10, colinear_chaining=False, selection_method=method, e_cutoff=e_cutoff)
        _assert_equals_model(got, model, inputs.reads)
        _assert_nothing_chained(got, len(inputs.reads))
        want = [inputs.select(model[r][0], method, len(inputs.reads[r]), e_cutoff) for r in range(len(inputs.reads))]
        print("e_cutoff", e_cutoff, "selected:", [_selected(got, r) for r in range(len(inputs.reads))], "model:", want)
        assert [_selected(got, r) for r in range(len(inputs.reads))] == want
    assert sum(len(w) for w in want) < sum(len(m[0]) for m in model)           # the cut-off dropped something


def test_without_chaining_through_the_seeded_entry(gca, inputs):   # noqa: F811
    model = inputs.run(True)
    for method in (gm.GREEDY_LENGTH, gm.SCHEDULE_SCORE, gm.ALL):
        got = _seeded_run(gca, inputs, colinear_chaining=False, selection_method=method)
        _assert_equals_model(got, model, inputs.seeded_reads)
        _assert_nothing_chained(got, len(inputs.seeded_reads))
        assert [_selected(got, r) for r in range(len(inputs.seeded_reads))] == [inputs.select(model[r][0], method, len(inputs.seeded_reads[r])) for r in range(len(inputs.seeded_reads))]


@pytest.mark.parametrize("merge", [False, True])
def test_without_chaining_the_writers_give_the_selected_alignments(gca, inputs, merge):   # noqa: F811
    """device_output 1 and 2 (+ 4 for the vg::Path bytes the GAM / JSON writers wrap): one GAF line per selected alignment, a read's lines in alignmentStart order; the
    host encoder over kept traces writes the same text; a line of an alignment that a chaining-mode run also writes (a read whose whole-read alignments win there) is
    that run's line byte for byte; one JSON line and one GAM message per GAF line."""
    reads = inputs.reads
    names = [f"r{i}" for i in range(len(reads))]
    graph = gca.AlignmentGraph(inputs.gfa)
    seeder = gca.MinimizerSeeder(graph)
    mode = (2 if merge else 1) | 4
    chained = gca.Aligner(graph, seeder, long_pass=True, device_output=mode).align_reads(reads, gaf_names=names, cigar_match_mismatch_merge=merge)
    chained_lines = [l for l in chained["gaf"].split(b"\n")[:-1] if not chained["chained_better"][names.index(l.split(b"\t")[0].decode())]]
    model = inputs.run(False)
    shared = 0
    for method in (gm.GREEDY_LENGTH, gm.ALL):
        dev = gca.Aligner(graph, seeder, long_pass=True, device_output=mode, colinear_chaining=False, selection_method=method).align_reads(
            reads, gaf_names=names, cigar_match_mismatch_merge=merge, other_formats=True)
        host = gca.Aligner(graph, seeder, long_pass=True, keep_traces=True, colinear_chaining=False, selection_method=method).align_reads(
            reads, gaf_names=names, cigar_match_mismatch_merge=merge)
        assert dev["gaf"] == host["gaf"] and dev["gaf_chained_skipped"] == 0
        lines = dev["gaf"].split(b"\n")[:-1]
        spans = [(names.index(f[0].decode()), int(f[2]), int(f[3])) for f in (l.split(b"\t") for l in lines)]
        want = []
        for r in range(len(reads)):
            picked = inputs.select(model[r][0], method, len(reads[r]))
            # the selection's order, sorted by start as the reference sorts it: std::sort replayed twice (src/Aligner.cpp:1003,1023), which defines the order of tied starts
            want += [(r, model[r][0][picked[i]][0], model[r][0][picked[i]][1]) for i in output_order([model[r][0][i][0] for i in picked], inputs.std_sort)]
        assert spans == want
        if method == gm.GREEDY_LENGTH:
            assert [l for l in lines if not chained["chained_better"][names.index(l.split(b"\t")[0].decode())]] == chained_lines
        shared += sum(l in lines for l in chained_lines)
        assert all(l in lines for l in chained_lines)
        assert dev["json"].count(b"\n") == len(lines)
        assert sum(len(group) for group in decode_gam_stream(gzip.decompress(dev["gam"]))) == len(lines)
    print("lines shared with the chaining-mode run:", shared, "of", 2 * len(chained_lines))
    assert shared >= 6


def test_invalid_values_are_refused_by_name(gca, inputs):   # noqa: F811
    graph = gca.AlignmentGraph(inputs.gfa)
    seeder = gca.MinimizerSeeder(graph)
    cases = [
        (dict(seed_extend_density=0.0, colinear_chaining=False), "seed_extend_density"),
        (dict(seed_extend_density=-0.5, colinear_chaining=False), "seed_extend_density"),
        (dict(seed_extend_density=float("nan"), colinear_chaining=False), "seed_extend_density"),
        (dict(seed_extend_density=0.002), "seed_extend_density"),
        (dict(extra_heuristic=2), "extra_heuristic"),
        (dict(selection_method=8), "selection_method"),
        (dict(selection_method=-1), "selection_method"),
        (dict(colinear_chaining=2), "colinear_chaining"),
    ]
    for kw, said in cases:
        with pytest.raises(RuntimeError) as err:
            gca.Aligner(graph, seeder, long_pass=True, **kw).align_reads(inputs.reads[:2])
        assert "error -1" in str(err.value) and said in str(err.value), (kw, str(err.value))
    with pytest.raises(RuntimeError) as err:
        gca.Aligner(graph, seeder, long_pass=False, colinear_chaining=False).align_reads(inputs.reads[:2])
    assert "error -1" in str(err.value) and "colinear_chaining" in str(err.value) and "long_pass" in str(err.value)
    batch = gca.ReadBatch(inputs.seeded_reads)
    seeds = gca.SeedBatch(graph, batch, [[as_hit(s) for s in hits] for hits in inputs.seeded_hits])
    with pytest.raises(RuntimeError, match="seed_extend_density"):
        gca.Aligner(graph, None, long_pass=True, seed_extend_density=0.002).align_batch(batch, seeds=seeds)
    gca.Aligner(graph, seeder, long_pass=True, seed_extend_density=0.002, colinear_chaining=False).align_reads(inputs.reads[:2])
