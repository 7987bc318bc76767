"""Every extension mode on IUPAC graph nodes and on reads with lower case, N, U and IUPAC codes (tests/letters_inputs.py): the device against the modes' own
Python models through the harnesses of the modes' test files - exact equalities throughout -, against the oracle with the modes off, and a batch that holds reads
with a letter outside the alphabet. tests/test_letters_model.py shows on the CPU that these inputs put the models on ambiguous nodes often enough, and that with
every mode off the models are the oracle on them."""
import gzip
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import graphaligner_model as gm                                          # noqa: E402
import seeding_model                                                     # noqa: E402
from band_model import BandModel                                         # noqa: E402
from fastmode_model import fast_chained_alignment, path_to_trace         # noqa: E402
from global_model import GlobalModel                                     # noqa: E402
from letters_inputs import SETS                                          # noqa: E402
from precise_model import PreciseModel                                   # noqa: E402
from test_band_controls_gpu import assert_model_equal, device_per_read, device_run   # noqa: E402
from test_fast_mode_gpu import GAP, UNTOUCHED, World, assert_traces_equal_the_model, assert_untouched, raw_path_off   # noqa: E402
from test_global_alignment_gpu import _set_launch                        # noqa: E402
from test_gpu_parity import COMPARE_KEYS, LONG_KEYS, align_comparable, compare, gca, run_case   # noqa: E402,F401
from test_letters_model import inputs                                    # noqa: E402,F401  (the module's inputs, built once)
from test_seeding_model import std_sort                                  # noqa: E402,F401

pytestmark = pytest.mark.gpu


def _assert_equals_model(got, want, reads, whole_read):
    """Alignment start, end, score, every trace cell, the anchors with their paths; failed_assertion exactly where the model trips an assertion; no capacity_exceeded."""
    dev = device_per_read(got, len(reads))
    print("device (start, end, score):", [[a[:3] for a in alns] for alns, _ in dev], "anchors", [len(a) for _, a in dev])
    print("model  (start, end, score):", [None if w is None else [a[:3] for a in w[0]] for w in want], "anchors", [None if w is None else len(w[1]) for w in want])
    print("failed_assertion", got["failed_assertion"].tolist(), "capacity_exceeded", got["capacity_exceeded"].tolist())
    assert [bool(x) for x in got["failed_assertion"]] == [w is None for w in want]
    assert int(np.sum(got["capacity_exceeded"])) == 0
    assert_model_equal(got, [w if w is not None else ([], []) for w in want], reads, whole_read)


# ---- the modes off: the oracle judges
@pytest.mark.parametrize("slab", [False, True])
def test_with_the_modes_off_the_device_is_the_oracle(gca, inputs, monkeypatch, slab):   # noqa: F811
    if slab:
        monkeypatch.setenv("GC_EXTEND_SLAB", "1")
    got, want = run_case(gca, inputs.gfa, inputs.whole, long_pass=True)
    compare(got, want, COMPARE_KEYS + LONG_KEYS)
    assert not np.any(want["failed_assertion"]) and int(want["read_longall_off"][-1]) >= len(inputs.whole) - 2
    for r in inputs.no_seed_reads:                                         # U for T: empty, not failed
        assert int(got["read_seed_off"][r + 1] - got["read_seed_off"][r]) == 0 and not got["failed_assertion"][r]
    got, want = run_case(gca, inputs.gfa, inputs.fragments, long_pass=False, split_len=64, split_gap=64)
    compare(got, want, COMPARE_KEYS)
    assert int(want["read_anchor_off"][-1]) >= 40


# ---- the whole-read pass against the models
def _cell_limit(inputs, std_sort, which="whole", whole_read=True, split=35):   # noqa: F811
    _, unlimited = inputs.run(std_sort, BandModel, which, whole_read, split=split)
    cells = sorted(unlimited.slice_cells)
    return cells[len(cells) // 4]                                          # the lower quartile: three quarters of the slices reach it


WHOLE = {   # setting: (model class, the model's arguments, the device's)
    "ramp": (BandModel, dict(ramp_bandwidth=25), dict(ramp_bandwidth=25)),
    "cells": (BandModel, "limit", "limit"),
    "global": (GlobalModel, {}, dict(force_global=True)),
    "clip 0.66": (PreciseModel, dict(precise_clipping=0.66, x_drop=0), dict(precise_clipping=0.66, x_drop=0)),
    "clip 0.66 xdrop 5": (PreciseModel, dict(precise_clipping=0.66, x_drop=5), dict(precise_clipping=0.66, x_drop=5)),
    "clip 0.7": (PreciseModel, dict(precise_clipping=0.7, x_drop=0), dict(precise_clipping=0.7, x_drop=0)),
    "global clip 0.66": (PreciseModel, dict(force_global=True, precise_clipping=0.66), dict(force_global=True, precise_clipping=0.66)),
}
FOUR, TWO = ["default", "force_fallback", "reg_cap", "no_column_store"], ["default", "force_fallback"]
WHOLE_CASES = [(s, l) for s, launches in (("ramp", TWO), ("cells", TWO), ("global", FOUR), ("clip 0.66", FOUR), ("clip 0.66 xdrop 5", FOUR), ("clip 0.7", FOUR),
                                         ("global clip 0.66", TWO)) for l in launches]


@pytest.mark.parametrize("setting,launch", WHOLE_CASES)
def test_whole_read_pass_equals_the_model(gca, inputs, monkeypatch, std_sort, setting, launch):   # noqa: F811
    cls, model_kw, device_kw = WHOLE[setting]
    if model_kw == "limit":
        model_kw = device_kw = dict(max_cells_per_slice=_cell_limit(inputs, std_sort))
    kw = _set_launch(monkeypatch, launch)
    got = device_run(gca, inputs.gfa, inputs.whole, True, bandwidth=10, **device_kw, **kw)
    want, ext = inputs.run(std_sort, cls, "whole", True, **model_kw)
    _assert_equals_model(got, want, inputs.whole, True)
    cells, on_ambiguous, letters = inputs.trace_letters(want)
    print("trace cells", cells, "on ambiguous nodes", on_ambiguous, "letters", letters, "counters_long", got["counters_long"].tolist())
    assert on_ambiguous >= 0.10 * cells > 0                                # what was compared lay on IUPAC nodes
    if "precise_clipping" in device_kw:
        assert not np.any(got["flatten_ties"]) and not np.any(got["flatten_ties_long"])
    if setting == "cells":
        assert any(c >= model_kw["max_cells_per_slice"] for c in ext.slice_cells)
    if setting == "ramp":
        assert ext.fired.get("ramp: rewind", 0) > 0
    if launch == "default" and setting in ("ramp", "global"):
        assert int(got["counters_long"][7]) == 0                           # nothing went to the plain-layout fallback


# ---- the fragment pass against the models
FRAGMENT = {
    "ramp": (BandModel, dict(ramp_bandwidth=25), dict(ramp_bandwidth=25)),
    "cells": (BandModel, "limit", "limit"),
    "global": (GlobalModel, {}, dict(force_global=True)),
    "clip 0.66": (PreciseModel, dict(precise_clipping=0.66, x_drop=0), dict(precise_clipping=0.66, x_drop=0)),
    "clip 0.66 xdrop 5": (PreciseModel, dict(precise_clipping=0.66, x_drop=5), dict(precise_clipping=0.66, x_drop=5)),
}


@pytest.mark.parametrize("setting,slab", [(s, slab) for s in ("ramp", "cells", "global") for slab in (False, True)] + [("clip 0.66", False), ("clip 0.66 xdrop 5", False)])
def test_fragment_pass_equals_the_model(gca, inputs, monkeypatch, std_sort, setting, slab):   # noqa: F811
    """64-base fragments, without the whole-read pass. The lockstep kernel declines every extension that touches an ambiguous node, so an anchor with such a node in its
    path came from k_extend_slab_band (k_extend_slab_clip under clipping, where the lockstep kernel is off): the model's anchors hold such paths, and the device's
    are equal to them. (The result carries no count of declined extensions.)"""
    if slab:
        monkeypatch.setenv("GC_EXTEND_SLAB", "1")
    cls, model_kw, device_kw = FRAGMENT[setting]
    if model_kw == "limit":
        model_kw = device_kw = dict(max_cells_per_slice=_cell_limit(inputs, std_sort, "fragments", False, 64))
    got = device_run(gca, inputs.gfa, inputs.fragments, False, bandwidth=10, split_len=64, split_gap=64, **device_kw)
    want, ext = inputs.run(std_sort, cls, "fragments", False, split=64, **model_kw)
    _assert_equals_model(got, want, inputs.fragments, False)
    anchors, with_ambiguous = inputs.anchor_paths(want)
    print("anchors", anchors, "with an ambiguous node in the path", with_ambiguous, "counters", got["counters"].tolist())
    assert with_ambiguous >= 0.15 * anchors > 0
    dev_anchors, dev_ambiguous = inputs.anchor_paths(device_per_read(got, len(inputs.fragments)))
    assert (dev_anchors, dev_ambiguous) == (anchors, with_ambiguous)
    if setting == "cells":
        assert any(c >= model_kw["max_cells_per_slice"] for c in ext.slice_cells)
    if "precise_clipping" in device_kw:
        assert not np.any(got["flatten_ties"])


# ---- --no-colinear-chaining
def _selected(got, r):
    return got["long_index"][int(got["read_long_off"][r]):int(got["read_long_off"][r + 1])].tolist()


@pytest.mark.parametrize("density,flag,method", [(0.0005, False, gm.ALL), (-1.0, True, gm.GREEDY_E)])
def test_without_chaining_equals_the_model(gca, inputs, std_sort, density, flag, method):   # noqa: F811
    """tests/graphaligner_model.py over the band model's extensions, as tests/test_graphaligner_mode_gpu.py: the alignments, the seeds extended and the selection."""
    _, _, g, original_size = inputs.world()
    model = gm.GraphAlignerModel(BandModel(g, 10), g, original_size)
    reads = inputs.whole
    graph_size = sum(g.length)
    want, full = [], []
    for read in reads:
        seeds = inputs.seeds(std_sort, read)
        alns, extended = model.align_one_way(read, seeds, True, seed_extend_density=density, extra_heuristic=flag) if seeds else ([], 0)
        want.append(([(a["start"], a["end"], a["score"], [tuple(c) for c in a["trace"]]) for a in alns], extended))
        full.append(model.align_one_way(read, seeds, True)[1] if seeds else 0)
    got = device_run(gca, inputs.gfa, reads, True, bandwidth=10, colinear_chaining=False, selection_method=method, seed_extend_density=density, extra_heuristic=flag)
    print("device (start, end, score):", [[a[:3] for a in alns] for alns, _ in device_per_read(got, len(reads))], "seeds extended", got["seeds_extended_long"].tolist())
    print("model  (start, end, score):", [[a[:3] for a in alns] for alns, _ in want], "seeds extended", [x[1] for x in want], "without the heuristics", full)
    assert not np.any(got["failed_assertion"]) and not np.any(got["capacity_exceeded"])
    assert_model_equal(got, [(alns, []) for alns, _ in want], reads, True)
    assert got["seeds_extended_long"].tolist() == [x[1] for x in want]
    assert [_selected(got, r) for r in range(len(reads))] == [gm.select_alignments([a[:3] for a in want[r][0]], method, graph_size, len(reads[r]), -1, std_sort) for r in range(len(reads))]
    assert int(got["read_anchor_off"][-1]) == 0 and got["chained_better"].tolist() == [0] * len(reads)
    if density > 0:
        assert sum(x[1] < f for x, f in zip(want, full)) >= 1              # the budget dropped seeds
    cells, on_ambiguous, _ = inputs.trace_letters([(alns, []) for alns, _ in want])
    assert on_ambiguous >= 0.10 * cells > 0


# ---- fast mode
class LettersWorld(World):
    """World of tests/test_fast_mode_gpu.py over this file's graph and reads. The graph letters the model compares are the oracle graph's own (the node sequences of
    tests/extension_model.py's Graph), and gc_graph_letters is held to them."""

    def __init__(self, gca, inputs):   # noqa: F811
        self.gca, self.inputs = gca, inputs
        self.gfa, self.reads = inputs.gfa, inputs.whole
        self.names = [f"r{i}" for i in range(len(self.reads))]
        self.graph = gca.AlignmentGraph(self.gfa)
        self.seeder = gca.MinimizerSeeder(self.graph)
        self.node_length = self.graph.array("nodeLength")
        self.node_ids = self.graph.array("nodeIDs")
        self.node_offset = self.graph.array("nodeOffset")
        self.base, want = run_case(gca, self.gfa, self.reads, long_pass=False, colinear_gap=GAP)
        compare(self.base, want, COMPARE_KEYS)
        self.base_long, want_long = run_case(gca, self.gfa, self.reads, long_pass=True, colinear_gap=GAP)
        compare(self.base_long, want_long, COMPARE_KEYS + LONG_KEYS)
        self.model = self.models(self.base)
        self.model_long = self.models(self.base_long)

    def models(self, got, reads=None):
        reads = self.reads if reads is None else reads
        g = self.inputs.graph()
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
            assert bytes(text) == "".join(g.sequence[v][o] for v, o in cells).encode(), r
            out.append(fast_chained_alignment(path, first, last, x, y, read, self.node_length, self.node_ids, self.node_offset, lambda v, o: g.sequence[v][o]))
        return out


@pytest.fixture(scope="module")
def world(gca, inputs):   # noqa: F811
    return LettersWorld(gca, inputs)


@pytest.mark.parametrize("long_pass", [False, True])
def test_fast_mode_equals_the_model(world, inputs, long_pass):   # noqa: F811
    """The reference counts the cells whose graph letter differs from the read's as chars (src/Aligner.cpp:834-843, the comparison at :839), and the graph letter is what
    AlignmentGraph::NodeSequences returns (src/AlignmentGraph.cpp:754-793): for an ambiguous node the upper-case IUPAC code of its four masks (:769-789), for any other
    node one of "ACGT" (:762). So a lower-case read differs from the graph at every cell, and an R in the read equals only an R in the graph: what
    tests/fastmode_model.py computes, and k_fast_chain_score with it."""
    got = world.align(fast_mode=True, long_pass=long_pass, chain_traces=2 if long_pass else 1, keep_seeds=True)
    base = world.align(fast_mode=False, long_pass=long_pass, chain_traces=2 if long_pass else 1, keep_seeds=True)
    assert_untouched(got, base)
    base_oracle = world.base_long if long_pass else world.base                # (held to the oracle when the world was made)
    for key in UNTOUCHED:
        if key in base_oracle and key not in ("read_path_off", "path_node"):  # (run_case expands the stitched path)
            assert np.array_equal(np.asarray(base[key]), np.asarray(base_oracle[key])), key
    model = world.model_long if long_pass else world.model
    stitched = [m is not None for m in model]
    print("scores", [m[4] if m else None for m in model], "default mode's NW distances", base["chain_edit_distance"].tolist())
    assert got["chain_edit_distance"].tolist() == [m[4] if m else -1 for m in model]
    assert_traces_equal_the_model(got, model, stitched)                    # chain_traces 1 without the whole-read pass (every stitched read wins), 2 with it
    if long_pass:
        selected = np.diff(got["read_long_off"]) > 0
        assert got["chained_better"].tolist() == [int(m is not None and (not selected[r] or int(got["long_edit_distance"][r]) > m[4])) for r, m in enumerate(model)]
    else:
        assert got["chained_better"].tolist() == [int(s) for s in stitched]
    assert not np.any(got["capacity_exceeded"])
    amb = inputs.ambiguous()
    off = raw_path_off(base_oracle)
    crossing = [r for r in range(len(world.reads)) if stitched[r] and any(amb[int(v)] for v in base_oracle["path_nodes_raw"][off[r]:off[r + 1]])]
    lettered = [r for r in inputs.lowercase_reads + inputs.iupac_reads if stitched[r]]
    print("stitched pieces that cross an ambiguous node:", crossing, "traced reads in lower case or with a code:", lettered)
    assert crossing and lettered
    for r in inputs.lowercase_reads:                                       # every cell of a lower-case read differs
        if stitched[r]:
            assert model[r][4] == int(base["path_cells"][r])


# ---- the writers
@pytest.mark.parametrize("force_global", [False, True])
@pytest.mark.parametrize("device_output", [1, 2, 4])
def test_the_writers_on_codes(gca, inputs, std_sort, device_output, force_global):   # noqa: F811
    """gc_params::device_output against the host encoders over kept traces, under clipping (with the X-drop, or forced global: the two exclude each other). Match or
    mismatch in a GAF line is decided by IUPAC sets: the compared lines cross a graph code that holds the read's base and one that does not."""
    reads = inputs.whole
    names = [f"r{i}" for i in range(len(reads))]
    graph = gca.AlignmentGraph(inputs.gfa)
    seeder = gca.MinimizerSeeder(graph)
    merge = device_output == 2
    formats = ("json", "gam") if device_output == 4 else ("gaf",)
    mode = dict(precise_clipping=0.66, force_global=True) if force_global else dict(precise_clipping=0.66, x_drop=50)
    kw = dict(long_pass=True, chain_traces=1, **mode)
    dev = gca.Aligner(graph, seeder, device_output=device_output, **kw).align_reads(reads, gaf_names=names, cigar_match_mismatch_merge=merge, formats=formats)
    host = gca.Aligner(graph, seeder, keep_traces=True, **kw).align_reads(reads, gaf_names=names, cigar_match_mismatch_merge=merge, formats=formats)
    for f in formats:
        if f == "gam":
            assert gzip.decompress(dev[f]) == gzip.decompress(host[f])
        else:
            assert dev[f] == host[f], f
    for key in ("chained_better", "chain_edit_distance", "long_edit_distance", "failed_assertion"):
        assert np.array_equal(np.asarray(dev[key]), np.asarray(host[key])), key
    want, _ = inputs.run(std_sort, PreciseModel, "whole", True, **mode)
    g = inputs.graph()
    lines = {}
    for line in (dev["gaf"].split(b"\n")[:-1] if "gaf" in formats else []):
        lines.setdefault(line.split(b"\t")[0].decode(), []).append(line)
    checked, holding, not_holding = 0, 0, 0
    for r in range(len(reads)):
        if host["chained_better"][r] or host["failed_assertion"][r]:
            continue
        picked = [int(host["read_longall_off"][r]) + int(i) for i in host["long_index"][int(host["read_long_off"][r]):int(host["read_long_off"][r + 1])]]
        picked.sort(key=lambda a: int(host["longall_start"][a]))
        expect = []
        for a in picked:
            t0, t1 = int(host["long_trace_off"][a]), int(host["long_trace_off"][a + 1])
            trace = list(zip(host["long_trace_node"][t0:t1].tolist(), host["long_trace_offset"][t0:t1].tolist(), host["long_trace_seqpos"][t0:t1].tolist(),
                             [bool(x) for x in host["long_trace_switch"][t0:t1]]))
            assert trace in [t for _, _, _, t in want[r][0]], f"read {r}: the written alignment is not one of the model's"
            for node, off, seqpos, _ in trace:
                split = g.unitig_node(node, off)
                c = g.sequence[split][off - g.node_offset[split]]
                if c not in "ACGT":
                    base = chr(reads[r][seqpos]).upper().replace("U", "T")
                    holds = bool(set(SETS.get(base, "")) & set(SETS[c]))
                    holding, not_holding = holding + holds, not_holding + (not holds)
            expect.append(gca.api.format_gaf_trace(graph, names[r], reads[r], host["long_trace_node"][t0:t1], host["long_trace_offset"][t0:t1], host["long_trace_seqpos"][t0:t1],
                                                   host["long_trace_switch"][t0:t1], merge=merge))
        if "gaf" in formats:
            assert lines.get(names[r], []) == expect, names[r]
        checked += len(expect)
    print("alignments written from whole-read traces:", checked, "their cells on a code that holds the read's base:", holding, "that does not:", not_holding)
    assert checked >= 5 and holding >= 1 and not_holding >= 1


# ---- reads with a letter outside the alphabet
PER_READ = ["failed_assertion", "seeds_extended", "chain_score", "chain_edit_distance", "chained_better", "chain_aln_start", "chain_aln_end", "flatten_ties"]
PER_READ_LONG = ["long_edit_distance", "flatten_ties_long"]
LISTS = [("read_seed_off", ["seed_node", "seed_offset", "seed_seqpos", "seed_goodness"]),
         ("read_anchor_off", ["anchor_x", "anchor_y", "anchor_score", "anchor_first_node", "anchor_first_offset", "anchor_first_seqpos", "anchor_last_node", "anchor_last_offset",
                              "anchor_last_seqpos"]),
         ("read_chain_off", ["chain"]), ("read_path_off", ["path_node", "path_offset"]),
         ("read_chain_trace_off", ["chain_trace_node", "chain_trace_offset", "chain_trace_seqpos", "chain_trace_switch"])]
LISTS_LONG = [("read_longall_off", ["longall_start", "longall_end", "longall_score"]), ("read_long_off", ["long_start", "long_end", "long_score"])]
NESTED = [("read_anchor_off", "anchor_path_off", ["anchor_path"]), ("read_anchor_off", "anchor_trace_off", ["anchor_trace_node", "anchor_trace_offset", "anchor_trace_seqpos", "anchor_trace_switch"])]
NESTED_LONG = [("read_longall_off", "long_trace_off", ["long_trace_node", "long_trace_offset", "long_trace_seqpos", "long_trace_switch"])]


def _of_read(res, r, long_pass, skip=()):
    """Everything the result holds for read r, as plain lists."""
    out = {k: int(res[k][r]) for k in PER_READ + (PER_READ_LONG if long_pass else []) if k not in skip}
    for off, keys in LISTS + (LISTS_LONG if long_pass else []):
        a, b = int(res[off][r]), int(res[off][r + 1])
        for k in keys:
            if k not in skip:
                out[k] = np.asarray(res[k][a:b]).tolist()
    for off, inner, keys in NESTED + (NESTED_LONG if long_pass else []):
        a, b = int(res[off][r]), int(res[off][r + 1])
        for k in keys:
            if k not in skip:
                out[k] = [np.asarray(res[k][int(res[inner][i]):int(res[inner][i + 1])]).tolist() for i in range(a, b)]
    return out


def _flagged_batch(inputs):   # noqa: F811
    """(reads, indices of the reads with a letter CommonUtils::Complement asserts on - src/CommonUtils.cpp:130-132, every character outside its cases -, of the others)."""
    bb = inputs.bb
    long_read = bytearray(bb[20000:24300])
    long_read[4200] = ord("X")                                            # beyond base 4096: the second turn of a lane in k_pack_read_masks
    bad = {2: bb[6000:6150] + b"X" + bb[6151:6300], 5: b"*" + bb[7001:7300], 9: bb[13000:13127] + b"-", 14: b"X", 20: bytes(long_read)}
    reads, flagged = [], []
    valid = list(inputs.whole)
    while valid or bad:
        if len(reads) in bad:
            flagged.append(len(reads))
            reads.append(bad.pop(len(reads)))
        else:
            reads.append(valid.pop(0))
    return reads, flagged, [i for i in range(len(reads)) if i not in flagged]


def _assert_flagged_are_empty(got, flagged, long_pass):
    assert [i for i, f in enumerate(got["failed_assertion"]) if f] == flagged
    assert int(np.sum(got["capacity_exceeded"])) == 0
    for i in flagged:
        mine = _of_read(got, i, long_pass)
        for k, v in mine.items():
            if isinstance(v, list):
                assert v == [], (i, k)
        assert mine["seeds_extended"] == 0 and mine["chained_better"] == 0 and mine["chain_edit_distance"] == -1


@pytest.mark.parametrize("long_pass", [False, True])
def test_a_letter_outside_the_alphabet_flags_its_read_alone(gca, inputs, long_pass):   # noqa: F811
    """The oracle, as the reference, gives up the whole batch on such a letter; the device flags the read (failed_assertion) and returns nothing for it. Every other
    read has the oracle's result for the batch without the flagged reads."""
    from oracle import Oracle
    reads, flagged, valid = _flagged_batch(inputs)
    graph = gca.AlignmentGraph(inputs.gfa)
    seeder = gca.MinimizerSeeder(graph)
    keys = COMPARE_KEYS + (LONG_KEYS if long_pass else [])
    got = align_comparable(gca.Aligner(graph, seeder, keep_traces=True, keep_seeds=True, long_pass=long_pass, chain_traces=2), graph, reads)
    want = Oracle(inputs.gfa, long_pass=long_pass).align([reads[i] for i in valid])
    _assert_flagged_are_empty(got, flagged, long_pass)
    for k, i in enumerate(valid):
        mine, theirs = _of_read(got, i, long_pass), _of_read(want, k, long_pass)
        assert set(mine) >= {key for key in keys if not key.endswith("_off")}
        for key in mine:
            assert mine[key] == theirs[key], (i, key)
    assert int(want["read_anchor_off"][-1]) > 100
    # the flag on: everything of the other reads is what the batch without the flagged reads gives (which tests above hold to the model)
    kw = dict(keep_traces=True, keep_seeds=True, long_pass=long_pass, chain_traces=2, fast_mode=True)
    fast = align_comparable(gca.Aligner(graph, seeder, **kw), graph, reads)
    alone = align_comparable(gca.Aligner(graph, seeder, **kw), graph, [reads[i] for i in valid])
    _assert_flagged_are_empty(fast, flagged, long_pass)
    for k, i in enumerate(valid):
        assert _of_read(fast, i, long_pass) == _of_read(alone, k, long_pass), i
        assert _of_read(fast, i, long_pass, skip=("chain_edit_distance", "chained_better", "chain_aln_start", "chain_aln_end", "chain_trace_node", "chain_trace_offset",
                                                  "chain_trace_seqpos", "chain_trace_switch")).items() <= _of_read(want, k, long_pass).items(), i


def test_flagged_reads_write_no_line(gca, inputs):   # noqa: F811
    reads, flagged, valid = _flagged_batch(inputs)
    names = [f"r{i}" for i in range(len(reads))]
    graph = gca.AlignmentGraph(inputs.gfa)
    seeder = gca.MinimizerSeeder(graph)
    for kw in (dict(keep_traces=True), dict(device_output=1 | 4)):
        aligner = gca.Aligner(graph, seeder, long_pass=True, chain_traces=1, **kw)
        got = aligner.align_reads(reads, gaf_names=names, other_formats=True)
        alone = aligner.align_reads([reads[i] for i in valid], gaf_names=[names[i] for i in valid], other_formats=True)
        assert [i for i, f in enumerate(got["failed_assertion"]) if f] == flagged
        assert got["gaf"] == alone["gaf"] and got["json"] == alone["json"]
        assert gzip.decompress(got["gam"]) == gzip.decompress(alone["gam"])
        written = {line.split(b"\t")[0].decode() for line in got["gaf"].split(b"\n")[:-1]}
        assert written and not written & {names[i] for i in flagged}


def test_flagged_reads_through_the_seeded_entry(gca, inputs, std_sort):   # noqa: F811
    """gc_align_batch_seeded with hits for the valid reads only: the same reads are flagged, and the others are what the minimizer path gives - its own hits, from
    tests/seeding_model.py, which tests/test_seed_hits_gpu.py holds to the oracle's."""
    reads, flagged, valid = _flagged_batch(inputs)
    graph_arrays, index, _, _ = inputs.world()
    hits = [[] if i in flagged else [(s["nodeID"], s["nodeOffset"], s["seqPos"], s["matchLen"], s["raw"], int(s["reverse"]))
                                     for s in seeding_model.get_seeds(read, index, graph_arrays, 15, 20, 10.0, std_sort)] for i, read in enumerate(reads)]
    graph = gca.AlignmentGraph(inputs.gfa)
    batch = gca.ReadBatch(reads)
    kw = dict(keep_traces=True, keep_seeds=True, long_pass=True, chain_traces=2)
    seeded = gca.Aligner(graph, None, **kw).align_batch(batch, seeds=gca.SeedBatch(graph, batch, hits))
    own = gca.Aligner(graph, gca.MinimizerSeeder(graph), **kw).align_batch(batch)

    def normal(out):
        from test_gpu_parity import expand_stitched_path, mark_missing_chain_alignments
        got = {k: (v.astype(np.int64) if isinstance(v, np.ndarray) and v.dtype.kind in "ui" and k not in ("counters", "counters_long") else v) for k, v in out.items()}
        expand_stitched_path(got, graph.array("nodeLength"))
        mark_missing_chain_alignments(got)
        sel = np.repeat(got["read_longall_off"][:-1], np.diff(got["read_long_off"])) + got["long_index"]
        for key in ("start", "end", "score"):
            got["long_" + key] = got["longall_" + key][sel]
        return got
    seeded, own = normal(seeded), normal(own)
    _assert_flagged_are_empty(seeded, flagged, True)
    _assert_flagged_are_empty(own, flagged, True)
    assert sum(len(h) for h in hits) == int(own["read_seed_off"][-1]) > 0
    for i in valid:
        assert _of_read(seeded, i, True) == _of_read(own, i, True), i
