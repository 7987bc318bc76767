"""The forced global alignment on the device (gc_params::force_global, the reference's --global-alignment): both extension passes against
tests/global_model.py through tests/alignment_model.py - the oracle has no such option -, the stages behind them by their own properties, and
the flag switched off against the oracle."""
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import seeding_model                                                     # noqa: E402
from alignment_model import AlignmentModel                               # noqa: E402
from band_model import BandModel                                         # noqa: E402
from extension_model import Graph                                        # noqa: E402
from global_model import GlobalModel                                     # noqa: E402
from test_band_controls_gpu import assert_model_equal, device_per_read, device_run   # noqa: E402
from test_gpu_parity import COMPARE_KEYS, LONG_KEYS, compare, gca, run_case   # noqa: E402,F401
from test_seeding_model import _inputs, std_sort                         # noqa: E402,F401

pytestmark = pytest.mark.gpu

LAUNCHES = ["default", "reg_cap", "force_fallback", "no_column_store"]


class Inputs:
    """The graph and the reads of this file, built once: SynthGraph(40_000, seed=23, repeats=3) and reads made from its backbone."""

    def __init__(self, directory):
        from graphchainer_amd.synth import SynthGraph
        self.sg = sg = SynthGraph(40_000, seed=23, repeats=3)
        self.gfa = os.path.join(str(directory), "g.gfa")
        sg.write_gfa(self.gfa)
        bb = self.bb = sg.backbone.tobytes()
        rng = random.Random(3)

        def rnd(n):
            return bytes(rng.choice(b"ACGT") for _ in range(n))

        def anti(a, n):      # letters that match the backbone on none of the diagonals -2..+2 where one is left, else none of -1..+1
            out = bytearray()
            for i in range(a, a + n):
                near, wide = set(bb[i - 1:i + 2]), set(bb[i - 2:i + 3])
                out.append(([c for c in b"ACGT" if c not in wide] or [c for c in b"ACGT" if c not in near] or [bb[i] ^ 6])[0])
            return bytes(out)

        def patchy(a, n, exact, w, junk):   # every w-base window: `exact` backbone bases, then junk(position, count)
            return b"".join(bb[l:l + exact] + junk(l + exact, w - exact) for l in range(a, a + n, w))

        self.whole = sg.sample_reads(3, 700, seed=9, p_del=0.07, p_sub=0.08, p_ins=0.07) + [
            bb[4000:4500] + bb[20000:20500],                                   # a chimera
            bb[30000:30300] + rnd(600),
            rnd(500) + bb[10000:10200],
            bb[12000:12200] + rnd(300) + bb[12500:12700],
            patchy(22000, 700, 17, 35, lambda a, n: rnd(n)),
            bb[26000:26200] + patchy(26200, 350, 17, 35, lambda a, n: rnd(n)),
            bb[15000:15064],                                                   # exactly one slice, no partial last slice
            bb[16000:16128],
            bb[17000:17050],                                                   # one partial slice
        ]
        self.long_trace = [bb[2000:2100] + anti(2100, 1500)]
        self.fragments = [
            patchy(22000, 640, 20, 64, anti),
            patchy(5000, 640, 24, 64, anti),
            rnd(3) + patchy(9000, 640, 18, 64, anti),
            patchy(30000, 320, 22, 64, anti) + bb[30320:30640],
        ]
        self._models = {}

    def model(self, std_sort, reads, cls, bandwidth, whole_read, split_len=35, split_gap=35, **band):
        """Per read: the whole-read alignments (start, end, score, trace) and the anchors (x, y, score, path) of AlignmentModel over `cls`; computed once per setting."""
        key = (id(reads), cls.__name__, bandwidth, whole_read, split_len, split_gap, tuple(sorted(band.items())))
        if key not in self._models:
            self._models[key] = model_results(self.gfa, reads, std_sort, cls, bandwidth, whole_read, split_len, split_gap, **band)
        return self._models[key]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    return Inputs(tmp_path_factory.mktemp("global"))


def model_results(gfa, reads, std_sort, cls, bandwidth, whole_read, split_len=35, split_gap=35, **band):
    from oracle import Oracle
    oracle = Oracle(gfa, long_pass=False)
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
    ext = cls(g, bandwidth, **band)
    model = AlignmentModel(ext, g, original_size)
    out = []
    for read in reads:
        seeds = seeding_model.order_seeds_by_chaining(seeding_model.get_seeds(read, index, graph, 15, 20, 10.0, std_sort), graph, std_sort)
        alns = []
        if whole_read and seeds:
            got, _ = model.align_one_way(read, seeds, True)
            alns = [(a["start"], a["end"], a["score"], [tuple(c) for c in a["trace"]]) for a in got]
        anchors = [(x, y, score, list(path)) for (x, y, path, first, last, score)
                   in model.anchors_of_read(read, seeding_model.fragment_order(seeds, std_sort), split_len=split_len, split_gap=split_gap)]
        out.append((alns, anchors))
    return out, ext


def _set_launch(monkeypatch, launch):
    kw = {}
    if launch == "reg_cap":
        monkeypatch.setenv("GC_TEST_LONG_REG_CAP", "3")
    elif launch == "force_fallback":
        monkeypatch.setenv("GC_TEST_LONG_FORCE_FALLBACK", "1")
    elif launch == "no_column_store":
        kw["capacities"] = {"long_column_store": -1}
    return kw


def _assert_end_to_end(got, reads):
    dev = device_per_read(got, len(reads))
    for r, read in enumerate(reads):
        if got["failed_assertion"][r]:
            continue
        for start, end, score, trace in dev[r][0]:
            assert (start, end) == (0, len(read)), f"read {r}: alignment ({start}, {end}) of {len(read)} bases"
    assert int(np.sum(got["capacity_exceeded"])) == 0
    assert int(np.sum(got["failed_assertion"])) <= 1


@pytest.mark.parametrize("launch", LAUNCHES)
def test_whole_read_pass_equals_the_model(gca, inputs, monkeypatch, std_sort, launch):
    reads = inputs.whole
    kw = _set_launch(monkeypatch, launch)
    got = device_run(gca, inputs.gfa, reads, True, bandwidth=10, force_global=True, **kw)
    want, ext = inputs.model(std_sort, reads, GlobalModel, 10, True)
    print("whole-read alignments (start, end, score):", [[a[:3] for a in alns] for alns, _ in device_per_read(got, len(reads))])
    print("failed_assertion", got["failed_assertion"].tolist(), "capacity_exceeded", got["capacity_exceeded"].tolist(), "counters_long", got["counters_long"].tolist())
    assert_model_equal(got, want, reads, True)
    _assert_end_to_end(got, reads)
    if launch == "default":
        assert int(got["counters_long"][7]) == 0                        # nothing went to the plain-layout fallback
    assert any(rule.startswith("global:") for rule in ext.fired)
    default, _ = inputs.model(std_sort, reads, BandModel, 10, True)
    differ = sum([a[:3] for a in want[r][0]] != [a[:3] for a in default[r][0]] for r in range(len(reads)))
    print("reads whose alignments differ from the default's:", differ)
    assert differ >= 3


def test_whole_read_pass_with_the_ramp_equals_the_model(gca, inputs, std_sort):
    """Nothing rewinds, so slice 0 alone runs at the ramp bandwidth."""
    reads = inputs.whole
    got = device_run(gca, inputs.gfa, reads, True, bandwidth=5, ramp_bandwidth=14, force_global=True)
    want, ext = inputs.model(std_sort, reads, GlobalModel, 5, True, ramp_bandwidth=14)
    print("whole-read alignments (start, end, score):", [[a[:3] for a in alns] for alns, _ in device_per_read(got, len(reads))])
    print("failed_assertion", got["failed_assertion"].tolist(), "capacity_exceeded", got["capacity_exceeded"].tolist(), "counters_long", got["counters_long"].tolist())
    assert_model_equal(got, want, reads, True)
    _assert_end_to_end(got, reads)
    assert "ramp: rewind" not in ext.fired


def test_a_long_tail_kept_past_the_hmm_cut_equals_the_model(gca, inputs, std_sort):
    """100 backbone bases, then 1500 that match nothing near their diagonal (1600 in all): the default stops after the backbone part, the forced run carries a
    score of hundreds to the read's end. An extension's trace has at most rows + 1 + score cells, which is what the whole-read pass reserves with the flag
    (2 * len + 2 and slack, where the default keeps 1.5 * len + 512).
    Measured on the model: the trace of this read has 1661 cells at a score of 859 (the default's room would be 2912). Only the horizontal steps add cells to
    the one per row, and the steps of a best alignment are mostly diagonal mismatches: 61 horizontal ones here. A longer tail does not change that - a tail of
    4500 bases made of the backbone with two of every five bases left out gave 4780 cells at a score of 2192, against room for 7412 - since junk aligns to
    junk at about half an edit per base, a bound on the horizontal steps too. So no input was found whose trace outgrows the default's room; the test checks
    what the long tail does exercise: hundreds of slices kept past the HMM's cut, on the device as in the model, with nothing refused for capacity."""
    reads = inputs.long_trace
    want, ext = inputs.model(std_sort, reads, GlobalModel, 10, True)
    default, _ = inputs.model(std_sort, reads, BandModel, 10, True)
    print("model: (start, end, score, trace cells)", [a[:3] + (len(a[3]),) for a in want[0][0]], "default", [a[:3] for a in default[0][0]],
          "room without the flag", len(reads[0]) + len(reads[0]) // 2 + 512)
    assert [a[:2] for a in want[0][0]] == [(0, len(reads[0]))]
    assert all(a[1] < 200 for a in default[0][0])
    assert ext.fired.get("global: kept past not correct-from-correct", 0) > 0
    got = device_run(gca, inputs.gfa, reads, True, bandwidth=10, force_global=True)
    assert not got["failed_assertion"][0]
    assert_model_equal(got, want, reads, True)
    assert int(np.sum(got["capacity_exceeded"])) == 0


@pytest.mark.parametrize("slab", [False, True])
def test_fragment_pass_equals_the_model(gca, inputs, monkeypatch, std_sort, slab):
    """64-base fragments: no extension of 34 rows or fewer reaches the score of 28 at which the default drops a one-slice extension."""
    if slab:
        monkeypatch.setenv("GC_EXTEND_SLAB", "1")
    reads = inputs.fragments
    got = device_run(gca, inputs.gfa, reads, False, bandwidth=10, force_global=True, split_len=64, split_gap=64)
    want, _ = inputs.model(std_sort, reads, GlobalModel, 10, False, 64, 64)
    dev = device_per_read(got, len(reads))
    print("anchors per read", [len(a) for _, a in dev], "top scores", [max([s for _, _, s, _ in a] or [-1]) for _, a in dev], "model", [len(a) for _, a in want])
    print("failed_assertion", got["failed_assertion"].tolist(), "capacity_exceeded", got["capacity_exceeded"].tolist(), "counters", got["counters"].tolist())
    assert not np.any(got["failed_assertion"])
    assert_model_equal(got, want, reads, False)
    assert int(np.sum(got["capacity_exceeded"])) == 0
    assert max(score for _, anchors in dev for _, _, score, _ in anchors) >= 28
    default, _ = inputs.model(std_sort, reads, BandModel, 10, False, 64, 64)
    print("default anchors per read", [len(a) for _, a in default])
    for r in range(len(reads)):
        assert default[r][1] != want[r][1], f"read {r}: the default gives the same anchors"


def _gaf_segments(gfa):
    return {f[1]: f[2] for f in (line.rstrip("\n").split("\t") for line in open(gfa)) if f[0] == "S"}


def _spell(path, segments):
    comp = {"A": "T", "T": "A", "C": "G", "G": "C"}
    out, at = [], 0
    while at < len(path):
        end = at + 1
        while end < len(path) and path[end] not in "<>":
            end += 1
        s = segments[path[at + 1:end]]
        out.append(s if path[at] == ">" else "".join(comp.get(c, c) for c in reversed(s)))
        at = end
    return "".join(out)


@pytest.mark.parametrize("merge", [False, True])
def test_downstream_stages_stay_consistent(gca, inputs, merge):
    """The device's own GAF pieces (gc_params::device_output 1: = / X items, 2: M items - the two are exclusive, so each is a case) against the host encoder
    over kept traces, and the lines by their own properties."""
    reads = inputs.whole
    names = [f"r{i}" for i in range(len(reads))]
    graph = gca.AlignmentGraph(inputs.gfa)
    seeder = gca.MinimizerSeeder(graph)
    dev = gca.Aligner(graph, seeder, long_pass=True, chain_traces=1, device_output=2 if merge else 1, force_global=True).align_reads(
        reads, gaf_names=names, cigar_match_mismatch_merge=merge)
    host = gca.Aligner(graph, seeder, long_pass=True, chain_traces=1, keep_traces=True, force_global=True).align_reads(
        reads, gaf_names=names, cigar_match_mismatch_merge=merge)
    assert dev["gaf"] == host["gaf"]
    for key in ("chained_better", "chain_edit_distance", "long_edit_distance", "failed_assertion"):
        assert np.array_equal(np.asarray(dev[key]), np.asarray(host[key])), key
    assert int(np.sum(dev["capacity_exceeded"])) == 0
    segments = _gaf_segments(inputs.gfa)
    first_line, lines = {}, 0
    for line in dev["gaf"].decode().splitlines():
        f = line.split("\t")
        r = names.index(f[0])
        if not dev["chained_better"][r]:                                       # a whole-read alignment: end to end
            assert (int(f[1]), int(f[2]), int(f[3])) == (len(reads[r]), 0, len(reads[r])), line[:80]
            lines += 1
        first_line.setdefault(r, f)
    print("GAF lines of whole-read alignments:", lines, "chained_better", np.asarray(dev["chained_better"]).tolist())
    assert lines >= 3                                                          # (the three backbone reads at least: nothing beats a distance of 0)
    # the path of a read's first line, spelled through the GFA, against the read: the NW distance the result reports (the first selected / the chained alignment's)
    order = sorted(first_line)
    parts = [_spell(first_line[r][5], segments)[int(first_line[r][7]):int(first_line[r][8])].encode() for r in order]
    distances = [int(d) for d in gca.edit_distance(parts, [reads[r] for r in order])]
    reported = [int(dev["chain_edit_distance"][r]) if dev["chained_better"][r] else int(dev["long_edit_distance"][r]) for r in order]
    print("distances", distances, "reported", reported)
    assert distances == reported


def test_off_means_off(gca, inputs):
    reads = inputs.whole
    got, want = run_case(gca, inputs.gfa, reads, long_pass=True)
    off = device_run(gca, inputs.gfa, reads, True, bandwidth=10, force_global=False)
    sel = np.repeat(off["read_longall_off"][:-1], np.diff(off["read_long_off"])) + off["long_index"]   # (as run_case: the selected alignments are indices into the read's list)
    for key in ("start", "end", "score"):
        off["long_" + key] = off["longall_" + key][sel]
    compare(got, want, COMPARE_KEYS + LONG_KEYS)
    compare(off, want, COMPARE_KEYS + LONG_KEYS)
    assert int(want["read_longall_off"][-1]) >= len(reads) - 1
    graph = gca.AlignmentGraph(inputs.gfa)
    seeder = gca.MinimizerSeeder(graph)
    with pytest.raises(RuntimeError, match="error -1"):
        gca.Aligner(graph, seeder, force_global=2).align_reads(reads[:2])
