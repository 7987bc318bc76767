"""The whole-read pass's rounds run on the stream of the device's token slot - one stream (highest priority, a hardware queue of its own) that the passes of every gc_stream use
in turn - while what comes before the token (init, the first round's select) and after it (the per-read results) runs on the pass's own stream. These are the places where the
hand-over between the two streams, or between two passes on the shared one, can go wrong: passes with little or no work, every launch shape of a round, the rounds' counts, and
two host threads taking the token in turn. Every result is held to the CPU oracle the way tests/test_gpu_parity.py::run_case does. (Queueing a round's extension ahead of its
work count, with a grid sized by a bound, was built and measured with these tests and not kept: DESIGN.md §11.)"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_gpu_parity import COMPARE_KEYS, LONG_KEYS, align_comparable, compare, gca, run_case   # noqa: E402,F401

pytestmark = pytest.mark.gpu

ALL_KEYS = COMPARE_KEYS + LONG_KEYS
HOOKS = ("GC_TEST_LONG_MAX_BLOCKS", "GC_TEST_LONG_SPECULATE", "GC_TEST_LONG_REG_CAP", "GC_TEST_LONG_TEAM", "GC_LONG_TOKEN", "GC_LONG_TOKENS")


class World:
    """One graph, one aligner, one oracle and the oracle's answers for the read sets the tests share (computed once, never changed)."""

    def __init__(self, gca, tmp):
        from graphchainer_amd.synth import SynthGraph
        from oracle import Oracle
        self.sg = SynthGraph(250_000, seed=5)
        self.gfa = str(tmp / "g.gfa")
        self.sg.write_gfa(self.gfa)
        self.graph = gca.AlignmentGraph(self.gfa)
        self.seeder = gca.MinimizerSeeder(self.graph)
        self.kw = dict(keep_traces=True, keep_seeds=True, long_pass=True, chain_traces=2)
        self.aligner = gca.Aligner(self.graph, self.seeder, **self.kw)
        self.oracle = Oracle(self.gfa, long_pass=True)
        self.reads200 = self.sg.sample_reads(200, 2500, seed=9)
        self.want200 = self.oracle.align(self.reads200)

    def run(self, reads):
        return align_comparable(self.aligner, self.graph, reads)


@pytest.fixture(scope="module")
def world(gca, tmp_path_factory):   # noqa: F811
    return World(gca, tmp_path_factory.mktemp("queued_rounds"))


@pytest.fixture(autouse=True)
def no_hooks(monkeypatch):
    for name in HOOKS:
        monkeypatch.delenv(name, raising=False)


def rounds_and_extensions(got):
    return int(got["counters_long"][6]), int(got["counters_long"][4])


def test_one_read_three_reads_and_a_pass_without_work(world):
    """Round 0 publishes few items (one read: two), fewer than two per read (one of three reads has no seed at all), or none: then no extension is launched, the token is never
    taken, the token's stream is never touched and the pass has no rounds."""
    seedless = b"A" * 1500                      # no minimizer of a homopolymer is in the graph
    one = world.sg.sample_reads(1, 3000, seed=41)
    three = world.sg.sample_reads(2, 2000, seed=42)
    three.insert(1, seedless)
    for reads in (one, three, [seedless]):
        got = world.run(reads)
        compare(got, world.oracle.align(reads), ALL_KEYS)
        seeds = np.diff(got["read_seed_off"])
        if reads is three:
            assert seeds[1] == 0 and seeds[0] > 0 and seeds[2] > 0
            assert np.diff(got["read_longall_off"])[1] == 0
        if len(reads) == 1 and reads[0] is seedless:
            assert seeds[0] == 0 and rounds_and_extensions(got) == (0, 0)
        else:
            # (a read aligned end to end by its first seed needs one round; the select behind it, on the token's stream, finds nothing)
            assert rounds_and_extensions(got)[0] >= 1


def test_persistent_waves_on_the_token_stream(world, monkeypatch):
    """GC_TEST_LONG_MAX_BLOCKS=7 caps every launch at seven waves: blocks x team < count, so the waves are persistent and fetch their items through the slot counter, which the
    retry launch behind them uses again. Per-read results equal the run without the hook and the oracle."""
    plain = world.run(world.reads200)
    monkeypatch.setenv("GC_TEST_LONG_MAX_BLOCKS", "7")
    capped = world.run(world.reads200)
    compare(plain, world.want200, ALL_KEYS)
    compare(capped, world.want200, ALL_KEYS)
    compare(capped, plain, ALL_KEYS + ["seeds_extended_long"])
    assert rounds_and_extensions(capped) == rounds_and_extensions(plain)
    assert rounds_and_extensions(plain)[0] >= 3
    monkeypatch.setenv("GC_TEST_LONG_TEAM", "4")   # (teams of four lanes: three waves hold twelve items, the rest is fetched in fours)
    monkeypatch.setenv("GC_TEST_LONG_MAX_BLOCKS", "3")
    compare(world.run(world.reads200), plain, ALL_KEYS + ["seeds_extended_long"])


def test_speculation_hook_from_round_zero(world, monkeypatch):
    """GC_TEST_LONG_SPECULATE=8: candidates per read and round from round 0 on, so every round holds the most items it can. The switch itself holds the value to 2
    (tests/test_switches_host.py), which keeps a round inside the work arrays; results equal the hook at 1 (one seed per round in every round) and the oracle."""
    monkeypatch.setenv("GC_TEST_LONG_SPECULATE", "8")
    wide = world.run(world.reads200)
    monkeypatch.setenv("GC_TEST_LONG_SPECULATE", "1")
    narrow = world.run(world.reads200)
    compare(wide, world.want200, ALL_KEYS)
    compare(narrow, world.want200, ALL_KEYS)
    compare(wide, narrow, ALL_KEYS + ["seeds_extended_long"])
    assert rounds_and_extensions(wide)[0] < rounds_and_extensions(narrow)[0]            # fewer rounds ...
    assert rounds_and_extensions(wide)[1] >= rounds_and_extensions(narrow)[1]           # ... for no fewer extensions


def test_retry_list_on_the_token_stream(world, gca, tmp_path, monkeypatch):   # noqa: F811
    """Work items whose band outgrows the register tables go on the round's retry list, which the two-lanes-per-wave launch behind the extension reads. A tangle (slices of more than 64 nodes: the graph tests/test_band_controls_gpu.py aligns against the oracle), and the register-table cap of the launch-shape tests
    (GC_TEST_LONG_REG_CAP=3: nearly every item is listed) with and without persistent waves."""
    from test_band_controls_gpu import MODEL_LONG_KEYS, _tangle_case
    gfa, reads = _tangle_case(tmp_path)
    got, want = run_case(gca, gfa, reads, long_pass=True)
    compare(got, want, COMPARE_KEYS + MODEL_LONG_KEYS)
    assert rounds_and_extensions(got)[0] >= 2
    monkeypatch.setenv("GC_TEST_LONG_REG_CAP", "3")
    compare(world.run(world.reads200), world.want200, ALL_KEYS)
    monkeypatch.setenv("GC_TEST_LONG_MAX_BLOCKS", "5")
    compare(world.run(world.reads200), world.want200, ALL_KEYS)


# rounds with work and extensions run (counters_long[6], [4]: bench.py's long_pass.rounds and long_pass.extensions_per_step) of the 500-read batch below, taken with the
# library of the parent commit 7207e50 ("Add a command line and a device FASTA/FASTQ loader"), whose rounds ran on a stream per gc_stream
PARENT_ROUNDS = 4
PARENT_EXTENSIONS = 3042


def test_round_and_work_counts_are_the_parents(gca, tmp_path):   # noqa: F811
    """The candidates-per-read rule, its inputs and so the number of rounds and of extensions are what they were. A graph with repeats and reads with
    structural variants, so that reads need several seeds and the tail rounds speculate."""
    from graphchainer_amd.synth import SynthGraph
    sg = SynthGraph(300_000, seed=17, repeats=3, repeat_len=1500)
    gfa = str(tmp_path / "g.gfa")
    sg.write_gfa(gfa)
    reads = sg.sample_reads(500, 3000, seed=77, sv_fraction=0.3, sv_len=600)
    got, want = run_case(gca, gfa, reads, long_pass=True)
    print("rounds, extensions:", rounds_and_extensions(got))
    compare(got, want, ALL_KEYS)
    # the cross-check that needs no device: every seed the pass extended ran at most two extensions (backward, forward), and speculation only adds to that
    assert rounds_and_extensions(got)[1] >= int(np.sum(got["seeds_extended_long"]))
    assert rounds_and_extensions(got) == (PARENT_ROUNDS, PARENT_EXTENSIONS)


def test_two_aligners_on_two_threads_share_the_token_stream(world, gca):   # noqa: F811
    """Two Aligners (two gc_streams) on two host threads over one device, four batches each: the passes take the token in turn and with it the one round stream of its slot.
    Every result equals the single aligner's and the oracle's."""
    from graphchainer_amd.workqueue import ReadQueue, run_queue
    read_sets = [world.sg.sample_reads(60, 2000, seed=51), world.sg.sample_reads(35, 3000, seed=52), world.sg.sample_reads(80, 1200, seed=53), world.sg.sample_reads(3, 2500, seed=54)]
    want = [world.oracle.align(rs) for rs in read_sets]
    single = [world.run(rs) for rs in read_sets]
    for s, w in zip(single, want):
        compare(s, w, ALL_KEYS)
    batches = [gca.ReadBatch(rs) for rs in read_sets]
    aligners = [gca.Aligner(world.graph, world.seeder, **world.kw) for _ in range(2)]
    from test_gpu_parity import _normalise
    node_length = world.graph.array("nodeLength")
    items = 8
    outs = run_queue(ReadQueue(items), lambda worker, item: aligners[worker].align_batch(batches[item % 4]), workers=2)
    assert sorted(i for i, _ in outs) == list(range(items))
    for item, out in outs:
        got = _normalise(out, node_length)
        compare(got, single[item % 4], ALL_KEYS + ["seeds_extended_long"])
        compare(got, want[item % 4], ALL_KEYS)
        assert rounds_and_extensions(got) == rounds_and_extensions(single[item % 4])
