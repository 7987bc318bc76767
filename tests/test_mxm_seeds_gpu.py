"""The device MUM / MEM seeder (gc_mxm_index_create + gc_seeds_mxm; MxmIndex / MxmIndex.seeds / SeedBatch.hits) against the brute-force model tests/mxm_model.py, as ordered lists:
  1. exact lists on a variant graph, min_len above, at and below the prefix table's 12 letters;
  2. windows with several occurrences (diverged repeats);
  3. intervals wider than a wave and than a block (homopolymers, STRs, a tandem array), then `count` cutting through ties;
  4. the hand-checked cases of tests/test_mxm_model.py with an empty read, a one-letter read and a flagged read in the batch;
  5. device-born seeds are ordinary seeds: the aligner's result from them equals its result from the same hits uploaded by the host;
  6. refusals, by name.
The hit counts asserted from the model are conditions on the inputs (taken with the model alone), so that a generator that drifts is noticed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import lowcomplexity as lc                                  # noqa: E402
import mxm_model as mm                                      # noqa: E402
from graphchainer_amd.synth import SynthGraph              # noqa: E402  (test inputs)
from test_gpu_parity import COMPARE_KEYS, LONG_KEYS, compare, expand_stitched_path, gca, mark_missing_chain_alignments   # noqa: E402,F401  (gca: the fixture)
from test_mxm_model import HAND_CASES                       # noqa: E402

pytestmark = pytest.mark.gpu

_COMP = bytes.maketrans(b"ACGT", b"TGCA")
_MODES = {"mem": mm.MEM, "mum": mm.MUM}
_SHARED = {}


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("mxm")


class Case:
    """A graph with its index, a read batch and the model's text: made once, shared by the tests that read them."""

    def __init__(self, gca, gfa, reads):   # noqa: F811
        self.gfa, self.reads = gfa, reads
        self.text = mm.Text(mm.gfa_segments(gfa))
        self.graph = gca.AlignmentGraph(gfa)
        self.index = gca.MxmIndex(self.graph)
        self.batch = gca.ReadBatch(reads)

    def device(self, mode, min_len, count=None):
        return [[tuple(h) for h in per_read.tolist()] for per_read in self.index.seeds(self.batch, mode, count=count, min_len=min_len).hits()]

    def model(self, mode, min_len, count=None, stats=None):
        return [mm.seeds(self.text, r, _MODES[mode], min_len, count, stats) for r in self.reads]


def variant_case(gca, workdir):   # noqa: F811
    if "variant" not in _SHARED:
        sg = SynthGraph(40_000, seed=37)
        gfa = str(workdir / "variant.gfa")
        sg.write_gfa(gfa)
        reads = sg.sample_reads(3, 1200, seed=6, p_del=0.01, p_sub=0.01, p_ins=0.01)
        reads.append(reads[0].translate(_COMP)[::-1])
        _SHARED["variant"] = Case(gca, gfa, reads)
    return _SHARED["variant"]


def test_exact_lists_across_the_prefix_table_boundary(gca, workdir):   # noqa: F811
    case = variant_case(gca, workdir)
    assert int(case.index.array("prefix_len")[0]) == 12
    counts = {}
    for mode in ("mem", "mum"):
        for min_len in (20, 12, 5):   # above the table's letters, at them, and the table-less binary search over the whole suffix array
            want = case.model(mode, min_len)
            counts[(mode, min_len)] = sum(len(w) for w in want[:3])
            assert case.device(mode, min_len) == want, (mode, min_len)
    assert (counts[("mem", 20)], counts[("mum", 20)], counts[("mem", 12)], counts[("mum", 12)]) == (69, 69, 116, 113)
    assert counts[("mem", 5)] > 100_000   # (every window of 5 letters is in the text hundreds of times)


def test_the_index_arrays_are_the_texts(gca, workdir):   # noqa: F811
    """The suffix array is a permutation of the text's positions in suffix order (checked on the model's text), and the segment table is the model's."""
    case = variant_case(gca, workdir)
    sa, starts, ids = case.index.array("sa"), case.index.array("node_start"), case.index.array("node_id")
    T = case.text.T
    assert starts.tolist() == case.text.starts and ids.tolist() == case.text.ids and len(sa) == len(T)
    assert np.array_equal(np.sort(sa), np.arange(len(T)))
    key = T.replace(b"$", b"!")   # the separator sorts before every letter
    step = max(1, len(sa) // 4000)
    for a, b in zip(sa[:-1:step].tolist(), sa[1::step].tolist()):
        assert key[a:] < key[b:]
    assert int(case.index.array("bytes")[0]) >= 4 * len(T) + (8 << 24)


def test_several_occurrences_per_position(gca, workdir):   # noqa: F811
    sg = SynthGraph(40_000, seed=37, repeats=3, repeat_len=2000, repeat_divergence=0.02)
    gfa = str(workdir / "repeats.gfa")
    sg.write_gfa(gfa)
    case = Case(gca, gfa, sg.sample_reads(6, 1200, seed=6, p_del=0.01, p_sub=0.01, p_ins=0.01))
    stats = {}
    mem, mum = case.model("mem", 20, stats=stats), case.model("mum", 20)
    assert (sum(map(len, mem)), sum(map(len, mum)), stats["widest"]) == (228, 127, 4)
    assert case.device("mem", 20) == mem
    assert case.device("mum", 20) == mum


def test_intervals_wider_than_a_wave_and_a_block_and_count_through_ties(gca, workdir):   # noqa: F811
    g, reads, _ = lc.tier("a")
    gfa = str(workdir / "tier_a.gfa")
    g.write_gfa(gfa)
    case = Case(gca, gfa, reads[:12])
    stats = {}
    mem, mum = case.model("mem", 12, stats=stats), case.model("mum", 12)
    assert (sum(map(len, mem)), sum(map(len, mum)), stats["widest"], sum(1 for w in mem for h in w if h[3] == 12)) == (102_232, 315, 629, 10_899)
    assert case.device("mem", 12) == mem
    assert case.device("mum", 12) == mum
    for count in (1, 100, 5000):
        want = [w[:count] for w in mem]   # the model's order is the defined one: the first `count` of it
        if count > 1:
            assert any(len(w) > count and w[count - 1][3] == w[count][3] for w in mem), count   # the cut goes through a tie
        assert case.device("mem", 12, count) == want, count
    assert case.device("mem", 12, 10**9) == mem
    assert case.device("mum", 12, 10) == [w[:10] for w in mum]


def test_edges(gca, workdir):   # noqa: F811
    """The hand cases' segments as one graph (so the lists are the model's on the whole text, not the hand-checked ones), their reads in one batch with an empty read, a read
    of one letter and a read with a letter outside the alphabet: that one is flagged and gets nothing, the others are unaffected."""
    segments = {}
    for _, segs, _, _, _, _, _ in HAND_CASES:
        segments.update(segs)
    segments[80] = "NN"   # nothing left after mapping
    gfa = str(workdir / "edges.gfa")
    with open(gfa, "w") as f:
        for i in sorted(segments):
            f.write(f"S\t{i}\t{segments[i]}\n")
    reads = sorted({c[2].encode() for c in HAND_CASES}) + [b"", b"A", b"GATTA-ACAC", b"acguACGTacgu"]
    case = Case(gca, gfa, reads)
    flagged = reads.index(b"GATTA-ACAC")
    for mode in ("mem", "mum"):
        for min_len in (2, 4, 5, 6, 8):
            for count in (None, 1, 2, 5):
                want = case.model(mode, min_len, count)
                assert want[flagged] == [] and want[reads.index(b"")] == [] and (min_len == 2 or want[reads.index(b"A")] == [])
                assert case.device(mode, min_len, count) == want, (mode, min_len, count)
    assert sum(len(w) for w in case.model("mem", 4)) > 20 and sum(len(w) for w in case.model("mum", 6)) >= 2


def _normalised(out, graph):
    """A result in the shape COMPARE_KEYS + LONG_KEYS name (what test_gpu_parity.run_case does before it compares)."""
    got = {k: (v.astype(np.int64) if isinstance(v, np.ndarray) and v.dtype.kind in "ui" and k not in ("counters", "counters_long") else v) for k, v in out.items()}
    expand_stitched_path(got, graph.array("nodeLength"))
    mark_missing_chain_alignments(got)
    sel = np.repeat(got["read_longall_off"][:-1], np.diff(got["read_long_off"])) + got["long_index"]
    for key in ("start", "end", "score"):
        got["long_" + key] = got["longall_" + key][sel]
    return got


def test_device_born_seeds_are_ordinary_seeds(gca, workdir):   # noqa: F811
    case = variant_case(gca, workdir)
    model_hits = case.model("mem", 20)
    uploaded = gca.SeedBatch(case.graph, case.batch, model_hits)
    assert [[tuple(h) for h in per_read.tolist()] for per_read in uploaded.hits()] == model_hits   # gc_seeds_hits gives back what was uploaded
    assert uploaded.kernel_ms == 0
    born = case.index.seeds(case.batch, "mem")
    assert born.kernel_ms > 0
    aligner = gca.Aligner(case.graph, None, keep_traces=True, keep_seeds=True, long_pass=True)
    got, want = _normalised(aligner.align_batch(case.batch, seeds=born), case.graph), _normalised(aligner.align_batch(case.batch, seeds=uploaded), case.graph)
    compare(got, want, COMPARE_KEYS + LONG_KEYS)
    assert int(got["read_anchor_off"][-1]) > 0 and int(got["read_longall_off"][-1]) > 0 and int(got["read_seed_off"][-1]) > 0
    plain = gca.Aligner(case.graph, None, keep_traces=True, keep_seeds=True, long_pass=True, colinear_chaining=False)
    got, want = plain.align_batch(case.batch, seeds=born), plain.align_batch(case.batch, seeds=uploaded)
    keys = [k for k in COMPARE_KEYS + LONG_KEYS if k in got] + ["long_index"]
    assert len(keys) > 30
    compare(got, want, keys)
    assert int(got["read_longall_off"][-1]) > 0


def test_refusals(gca, workdir):   # noqa: F811
    case = variant_case(gca, workdir)
    for kw, message in ((dict(min_len=1), "min_len must be at least 2"), (dict(min_len=0), "min_len must be at least 2"), (dict(count=0), "max_count must be at least 1"),
                        (dict(mode=3), "neither GC_MXM_MUM nor GC_MXM_MEM"), (dict(mode=0), "neither GC_MXM_MUM nor GC_MXM_MEM")):
        with pytest.raises(RuntimeError, match=message):
            case.index.seeds(case.batch, **kw)
    other_graph = gca.AlignmentGraph(case.gfa)   # the same file, another graph object
    with pytest.raises(RuntimeError, match="the index was built from another graph"):
        case.index.seeds(case.batch, "mem", graph=other_graph)
    other_batch = gca.ReadBatch([r + b"A" for r in case.reads])
    seeds = case.index.seeds(case.batch, "mem")
    aligner = gca.Aligner(case.graph, None, long_pass=True)
    with pytest.raises(RuntimeError, match="another read batch"):
        aligner.align_batch(other_batch, seeds=seeds)
    lib = gca.load_library()
    handle = C.c_void_p()
    assert lib.gc_seeds_mxm(case.graph.handle, case.index.handle, None, 2, 1, 20, C.byref(handle)) == -1 and b"null" in lib.gc_last_error()
    with pytest.raises(RuntimeError, match="unknown index array"):
        case.index.array("nope")
    assert case.device("mem", 20) == case.model("mem", 20)   # the index and the batch are what they were
