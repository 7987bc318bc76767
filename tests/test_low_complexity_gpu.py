"""The HIP path against the CPU oracle on low-complexity sequence and on very short reads, bit-exact on every key: homopolymers, short tandem repeats and tandem
arrays (tests/lowcomplexity.py), where one read carries tens of thousands of seeds, thousands of anchors and 20-165 whole-read alignments and the device-side tables
stop being comfortably oversized; tests/test_low_complexity.py shows with the oracle alone that the tiers sit where they claim."""
import gzip
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import lowcomplexity as lc                                                                    # noqa: E402
from test_gpu_parity import COMPARE_KEYS, LONG_KEYS, _normalise, _revcomp, compare, gca, run_case   # noqa: E402,F401  (gca: the fixture)

pytestmark = pytest.mark.gpu

ALL_KEYS = COMPARE_KEYS + LONG_KEYS
_CASES = {}     # (tier, split_gap) -> the oracle's results: the oracle runs once per graph and parameters, the product once per route


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("lowcomplexity")


def tier_case(workdir, name, split_gap):
    from oracle import Oracle
    if (name, split_gap) not in _CASES:
        g, reads, n_ordinary = lc.tier(name)
        gfa = str(workdir / f"{name}.gfa")
        if not os.path.exists(gfa):
            g.write_gfa(gfa)
        t0 = time.time()
        oracle = Oracle(gfa, long_pass=True, split_gap=split_gap)
        want = oracle.align(reads)
        paths_off = oracle.graph_array("paths_off")
        print(f"oracle: tier {name} split_gap {split_gap}: {time.time() - t0:.1f} s")
        _CASES[(name, split_gap)] = (gfa, reads, n_ordinary, want, int(np.diff(paths_off).max()))
    return _CASES[(name, split_gap)]


def product(gca, gfa, reads, split_gap=35, keep_traces=True, seeder_kw=None, **kw):   # noqa: F811
    """run_case's product half: long_pass, keep_seeds and the chained traces always on."""
    graph = gca.AlignmentGraph(gfa)
    seeder = gca.MinimizerSeeder(graph, **(seeder_kw or {}))
    aligner = gca.Aligner(graph, seeder, keep_traces=keep_traces, keep_seeds=True, long_pass=True, chain_traces=2, split_gap=split_gap, **kw)
    t0 = time.time()
    got = _normalise(aligner.align_reads(reads), graph.array("nodeLength"))
    got["wall_s"] = time.time() - t0
    return got


def report(label, got):
    """What DESIGN.md's "Low-complexity input" table records per run."""
    flagged = np.nonzero(np.asarray(got["capacity_exceeded"]))[0].tolist()
    print(f"{label}: {got['wall_s']:.2f} s, fragment pool reruns {int(got['counters'][6])}, host-stitched reads {int(got['counters'][7])}, whole-read rounds {int(got['counters_long'][6])}, "
          f"plain-layout reruns {int(got['counters_long'][7])}, most whole-read alignments {int(np.diff(got['read_longall_off']).max(initial=0))}, capacity_exceeded {flagged}, "
          f"failed_assertion {np.nonzero(np.asarray(got['failed_assertion']))[0].tolist()}")


def no_flags(got):
    assert not np.asarray(got["capacity_exceeded"]).any(), np.nonzero(np.asarray(got["capacity_exceeded"]))[0]
    assert not np.asarray(got["failed_assertion"]).any()


_PER_READ = ["chain_score", "failed_assertion", "seeds_extended", "long_edit_distance", "chain_edit_distance", "chained_better", "flatten_ties", "flatten_ties_long", "chain_aln_start", "chain_aln_end"]
_SEED_LISTS = [("read_seed_off", k) for k in ("seed_node", "seed_offset", "seed_seqpos", "seed_goodness")]
_ANCHOR_LISTS = [("read_anchor_off", k) for k in ("anchor_x", "anchor_y", "anchor_score", "anchor_first_node", "anchor_first_offset", "anchor_first_seqpos", "anchor_last_node", "anchor_last_offset", "anchor_last_seqpos")]
_OTHER_LISTS = [("read_chain_off", "chain"), ("read_path_off", "path_node"), ("read_path_off", "path_offset"),
                ("read_longall_off", "longall_start"), ("read_longall_off", "longall_end"), ("read_longall_off", "longall_score"), ("read_long_off", "long_start"), ("read_long_off", "long_end"), ("read_long_off", "long_score"),
                ("read_chain_trace_off", "chain_trace_node"), ("read_chain_trace_off", "chain_trace_offset"), ("read_chain_trace_off", "chain_trace_seqpos"), ("read_chain_trace_off", "chain_trace_switch")]
_NESTED = [("read_anchor_off", "anchor_path_off", ("anchor_path",)), ("read_anchor_off", "anchor_trace_off", ("anchor_trace_node", "anchor_trace_offset", "anchor_trace_seqpos", "anchor_trace_switch")),
           ("read_longall_off", "long_trace_off", ("long_trace_node", "long_trace_offset", "long_trace_seqpos", "long_trace_switch"))]


def assert_read_equal(got, r, want, wr, lists=None, scalars=True):
    """Read r of `got` against read wr of `want`, every array of ALL_KEYS cut down to the read."""
    for off, key in (_SEED_LISTS + _ANCHOR_LISTS + _OTHER_LISTS) if lists is None else lists:
        a = np.asarray(got[key][int(got[off][r]):int(got[off][r + 1])], dtype=np.int64)
        b = np.asarray(want[key][int(want[off][wr]):int(want[off][wr + 1])], dtype=np.int64)
        assert np.array_equal(a, b), (r, key)
    if lists is not None and not scalars:
        return
    for key in _PER_READ:
        assert int(got[key][r]) == int(want[key][wr]), (r, key)
    for off, inner, keys in _NESTED:
        a0, a1 = int(got[inner][int(got[off][r])]), int(got[inner][int(got[off][r + 1])])
        b0, b1 = int(want[inner][int(want[off][wr])]), int(want[inner][int(want[off][wr + 1])])
        for key in keys:
            assert np.array_equal(np.asarray(got[key][a0:a1], dtype=np.int64), np.asarray(want[key][b0:b1], dtype=np.int64)), (r, key)


@pytest.mark.parametrize("name,split_gap", [("a", 35), ("a", 18), ("b", 35), ("b", 18), ("c", 35), ("c", 18), ("d", 35), ("d", 18)])
def test_tiers_equal_the_oracle(gca, workdir, name, split_gap):   # noqa: F811
    """(a) homopolymers, STRs, an exact unit-12 array: reads with few or no seeds, reads that enter and leave a block (and, crossing a homopolymer, up to 144 whole-read
    alignments); (b) unit-2000 / unit-500 arrays under 10 kb reads: 340-4 100 anchors, both LDS classes of k_chain and its slot routing; (c) unit-64 / unit-150 arrays
    under 4-5 kb reads: 23-52 whole-read alignments, either side of the first 32 slots; (d) a unit-150 array of 12 kb under 10 kb reads: 26 k seeds, 7.5 k / 15 k anchors,
    82 and 107 alignments. No read is flagged: a read that outgrows its alignment slots runs again with more. The ordinary reads of the batch come out as in a batch of
    their own - one read's problem never costs the others."""
    gfa, reads, n_ordinary, want, _ = tier_case(workdir, name, split_gap)
    got = product(gca, gfa, reads, split_gap)
    report(f"tier {name} split_gap {split_gap}", got)
    compare(got, want, ALL_KEYS)
    no_flags(got)
    alone, want_alone = run_case(gca, gfa, reads[-n_ordinary:], long_pass=True, split_gap=split_gap)
    compare(alone, want_alone, ALL_KEYS)
    no_flags(alone)
    for i in range(n_ordinary):
        assert_read_equal(got, len(reads) - n_ordinary + i, alone, i)


ROUTES = [{"GC_EXT_LAZY": "0"}, {"GC_EXT_LAZY": "1"}, {"GC_EXTEND_SLAB": "1"}, {"GC_TEST_CHAIN_FORCE_SCRATCH": "1", "GC_CHAIN_PLAIN_SCAN": "0"}, {"GC_TEST_CHAIN_FORCE_SCRATCH": "1", "GC_CHAIN_PLAIN_SCAN": "1"},
          {"GC_TEST_LONG_FORCE_FALLBACK": "1"}, {"GC_TEST_LONG_FORCE_FALLBACK": "1", "GC_TEST_LONG_MAX_ALIGNMENTS": "2"}, {"GC_TEST_LONG_SPECULATE": "2"}]


@pytest.mark.parametrize("env", ROUTES, ids=lambda e: "-".join(f"{k[3:].lower()}={v}" for k, v in e.items()))
def test_kernel_routes_on_tandem_reads(gca, workdir, monkeypatch, env):   # noqa: F811
    """Tier (c) through the routes the suite forces elsewhere on ordinary reads: eager and lazy fragment extension (the same results, so each equals the oracle), the slab
    layout, k_chain's scratch launch with either scan, the plain-layout whole-read kernel (also from a first capacity of two alignments: the rounds grow the slots and the
    rerun by the plain-layout kernel finds them grown), speculative rounds."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    gfa, reads, _, want, _ = tier_case(workdir, "c", 35)
    got = product(gca, gfa, reads, 35)
    report(f"tier c {env}", got)
    compare(got, want, ALL_KEYS)
    no_flags(got)
    if "GC_TEST_LONG_FORCE_FALLBACK" in env:
        assert int(got["counters_long"][7]) == len(reads)


@pytest.mark.parametrize("host_anchors", ["0", "1"])
def test_anchor_arrays_of_tandem_reads_without_traces(gca, workdir, monkeypatch, host_anchors):   # noqa: F811
    monkeypatch.setenv("GC_HOST_ANCHORS", host_anchors)
    gfa, reads, _, want, _ = tier_case(workdir, "c", 35)
    got = product(gca, gfa, reads, 35, keep_traces=False)
    compare(got, want, [k for k in ALL_KEYS if "trace" not in k])
    no_flags(got)


def test_output_formats_of_tandem_reads(gca, workdir):   # noqa: F811
    """GAF, JSON and GAM of tier (c): k_out_encode (device_output 1 | 4) against the host encoders byte for byte, and the GAF and JSON against the oracle's writers."""
    from oracle import Oracle
    gfa, reads, _, want, _ = tier_case(workdir, "c", 35)
    graph = gca.AlignmentGraph(gfa)
    seeder = gca.MinimizerSeeder(graph)
    ids = [f"r{i}" for i in range(len(reads))]
    host = gca.Aligner(graph, seeder, keep_traces=2, long_pass=True).align_reads(reads, gaf_names=ids, other_formats=True)
    dev = gca.Aligner(graph, seeder, long_pass=True, device_output=1 | 4).align_reads(reads, gaf_names=ids, other_formats=True)
    oracle = Oracle(gfa, long_pass=True)
    oracle.align(reads)
    assert host["gaf"] == oracle.gaf(False) and host["json"] == oracle.json()
    assert dev["gaf"] == host["gaf"] and dev["json"] == host["json"] and gzip.decompress(dev["gam"]) == gzip.decompress(host["gam"])
    assert not np.asarray(dev["capacity_exceeded"]).any() and not np.asarray(host["capacity_exceeded"]).any()
    lines_per_read = np.bincount([int(line.split(b"\t")[0][1:]) for line in host["gaf"].splitlines() if line], minlength=len(reads))
    assert lines_per_read.min() >= 1, lines_per_read      # (of a tandem read's 23-52 alignments the selection keeps those that do not overlap: here the end-to-end one)


def test_the_read_nearest_the_16_bit_chain_limit(gca, workdir):   # noqa: F811
    """One 10 kb read inside a unit-64 array of 12 kb at split_gap 18 (17.7 k anchors, 28 k slots, 165 whole-read alignments) among ordinary reads. k_chain indexes a
    read's anchors and its entries (one per cover path through an anchor's end node) with 16 bits: the read may be flagged only if its anchors, or its anchors times the
    most cover paths through a node of the graph, exceed 65 535 - and then its seeds and anchors are still the oracle's and its chain is empty. Otherwise, and for
    every other read, everything equals the oracle's."""
    gfa, reads, n_ordinary, want, max_paths = tier_case(workdir, "limit", 18)
    got = product(gca, gfa, reads, 18)
    report("limit read, split_gap 18", got)
    flagged = np.asarray(got["capacity_exceeded"]).astype(bool)
    anchors = int(want["read_anchor_off"][1] - want["read_anchor_off"][0])
    print(f"limit read: {anchors} anchors x at most {max_paths} cover paths through a node = {anchors * max_paths}; flagged {flagged.tolist()}")
    assert not flagged[1:].any() and not np.asarray(got["failed_assertion"]).any()
    if flagged[0]:
        assert anchors > 65535 or anchors * max_paths > 65535
        assert_read_equal(got, 0, want, 0, lists=_SEED_LISTS + _ANCHOR_LISTS, scalars=False)
        assert int(got["read_chain_off"][1]) == int(got["read_chain_off"][0])
        for r in range(1, len(reads)):
            assert_read_equal(got, r, want, r)
    else:
        compare(got, want, ALL_KEYS)


def _short_reads(source, lengths):
    reads = []
    for n in lengths:
        reads += [source[3 * n:3 * n + n], _revcomp(source[3 * n + 7:3 * n + 7 + n])]
    return reads


def _short_read_classes(want, n):
    seeds, anchors, alns = np.diff(want["read_seed_off"]), np.diff(want["read_anchor_off"]), np.diff(want["read_longall_off"])
    return (seeds == 0) & (anchors == 0) & (alns == 0), (seeds > 0) & (anchors == 0), anchors > 0


@pytest.mark.parametrize("where", ["backbone", "unit150"])
def test_every_read_length_up_to_149(gca, workdir, tmp_path, where):   # noqa: F811
    """Every length 0-149, forward and reverse-complemented, in one batch: across k = 15, w = 20, split_len 35, the 64-row word and 2 x split_len, cut from the backbone
    of a plain 30 kbp graph and from inside a unit-150 array. The oracle alone says the sweep is not vacuous: some reads have nothing, some seeds but no anchor, some anchors."""
    from graphchainer_amd.synth import SynthGraph
    if where == "backbone":
        sg = SynthGraph(30_000, seed=61)
        gfa = str(tmp_path / "plain.gfa")
        sg.write_gfa(gfa)
        source = sg.backbone[4000:5000].tobytes()
    else:
        gfa = tier_case(workdir, "c", 35)[0]
        g = lc.tier("c")[0]
        b0 = g.blocks[1][2]
        source = g.sg.backbone[b0 + 600:b0 + 1600].tobytes()
    reads = _short_reads(source, range(150))
    got, want = run_case(gca, gfa, reads, long_pass=True)
    compare(got, want, ALL_KEYS)
    no_flags(got)
    nothing, seeds_only, anchored = _short_read_classes(want, len(reads))
    lengths = np.repeat(np.arange(150), 2)
    print(where, "first length with seeds", lengths[~nothing].min(), "with an anchor", lengths[anchored].min(), "reads with seeds and no anchor", int(seeds_only.sum()))
    assert nothing.sum() >= 2 * 15 and seeds_only.sum() >= 4 and anchored.sum() >= 100
    assert lengths[~nothing].min() >= 15 and lengths[anchored].min() >= 35
    if where == "backbone":
        # a batch of one: nothing may lean on a longer read having sized the batch's tables
        for n in (0, 1, 14, 15, 16, 17, 18, 19, 34, 35, 36, 37, 63, 64, 65, 66, 69, 70, 71, 72):
            for i in (2 * n, 2 * n + 1):
                one = product(gca, gfa, [reads[i]])
                no_flags(one)
                assert_read_equal(one, 0, want, i)


def test_short_reads_with_longer_minimizers(gca, tmp_path):   # noqa: F811
    """Lengths 0-80 with k = 19, w = 30: the first seed and the first anchor move with k and w."""
    from graphchainer_amd.synth import SynthGraph
    from oracle import Oracle
    sg = SynthGraph(30_000, seed=61)
    gfa = str(tmp_path / "plain.gfa")
    sg.write_gfa(gfa)
    reads = _short_reads(sg.backbone[4000:5000].tobytes(), range(81))
    got = product(gca, gfa, reads, seeder_kw={"minimizer_length": 19, "window_size": 30})
    want = Oracle(gfa, k=19, w=30, long_pass=True).align(reads)
    compare(got, want, ALL_KEYS)
    no_flags(got)
    nothing, seeds_only, anchored = _short_read_classes(want, len(reads))
    assert nothing.sum() >= 2 * 19 and seeds_only.sum() >= 10 and anchored.sum() >= 5 and np.repeat(np.arange(81), 2)[~nothing].min() >= 19


@pytest.mark.parametrize("cap", [1, 3, 24])
def test_first_alignment_capacity_boundary(gca, workdir, monkeypatch, capfd, cap):   # noqa: F811
    """GC_TEST_LONG_MAX_ALIGNMENTS makes the first capacity tiny, so ordinary reads take the rerun as well. A read with exactly as many alignments as slots fills them
    without asking for more; one more alignment and it runs again. Tier (a) holds reads with 0-4, 16, 18, 24, 34, 36, 40, 69 and 144 alignments: around each capacity here
    there are reads with one fewer, exactly as many and one more (23 / 24 / 25 taken from tier (c) as well). The reruns announce themselves under GC_DEBUG_TIMES."""
    monkeypatch.setenv("GC_TEST_LONG_MAX_ALIGNMENTS", str(cap))
    monkeypatch.setenv("GC_DEBUG_TIMES", "1")
    seen = set()
    for name in ("a", "c") if cap == 24 else ("a",):
        gfa, reads, _, want, _ = tier_case(workdir, name, 35)
        seen |= set(np.diff(want["read_longall_off"]).tolist())
        got = product(gca, gfa, reads, 35)
        report(f"first capacity {cap}, tier {name}", got)
        compare(got, want, ALL_KEYS)
        no_flags(got)
        reruns = capfd.readouterr().err.count("found more whole-read alignments than they had slots for")
        assert reruns >= (2 if name == "a" else 1), reruns          # 144 alignments from `cap` slots: several reruns, each with four times the slots
    assert {cap - 1, cap, cap + 1} <= seen, sorted(seen)


def test_plain_layout_reruns_grow_their_alignment_slots(gca, workdir, monkeypatch):   # noqa: F811
    """Reads the rounds hand to the plain-layout kernel unfinished (here: an extension scratch too small for any 3 kb read) meet the alignment capacity there for the first
    time; with a first capacity of one they are given more slots inside the rerun loop. Reads that the plain-layout kernel's four-fold room does not hold either are flagged,
    every other read equals the oracle."""
    monkeypatch.setenv("GC_TEST_LONG_MAX_ALIGNMENTS", "1")
    gfa, reads, _, want, _ = tier_case(workdir, "a", 35)
    got = product(gca, gfa, reads, 35, capacities={"long_max_items": 64})
    report("plain-layout reruns from one slot", got)
    flagged = np.asarray(got["capacity_exceeded"]).astype(bool)
    assert int(got["counters_long"][7]) > 0 and not np.asarray(got["failed_assertion"]).any()
    exact_with_several = 0
    for r in np.nonzero(~flagged)[0]:
        assert_read_equal(got, r, want, r)
        exact_with_several += int(want["read_longall_off"][r + 1] - want["read_longall_off"][r]) >= 2
    assert exact_with_several >= 2, (exact_with_several, flagged.tolist())
