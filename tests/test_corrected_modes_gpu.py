"""Corrected reads (gc_params::device_output & 8) and the order of a read's output under every alignment mode: without chaining and with each kind of selection,
through tied alignment starts (libstdc++'s std::sort replayed twice, tests/corrected_model.output_order), in fast mode, forced global, clipped, with the band controls,
through the seeded entry, and with one stream's buffers reused by calls of different size. The yardsticks are tests/corrected_model.py over the kept traces of the same
batch and, independently of any model, the letters of each GAF line's path. The read sets are those of the mode tests; their extension models are not run here."""
import gzip
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import corrected_model as cm                                                     # noqa: E402
import graphaligner_model as gm                                                  # noqa: E402
import lowcomplexity as lc                                                       # noqa: E402
import seeding_model                                                             # noqa: E402
from fastmode_model import path_to_trace                                         # noqa: E402
from test_corrected_gpu import COMPLEMENT, gfa_segments, letter_of, spell_gaf_line   # noqa: E402
from test_corrected_model import tie_shape                                       # noqa: E402
from test_fast_mode_gpu import GAP, make_reads                                   # noqa: E402
from test_global_alignment_gpu import Inputs                                     # noqa: E402
from test_gpu_parity import gca                                                  # noqa: E402,F401
from test_graphaligner_model import inputs as ga_inputs                          # noqa: E402,F401  (the reads of the mode without chaining, built once)
from test_precise_clipping_gpu import ClipInputs                                 # noqa: E402
from test_seeding_model import std_sort                                          # noqa: E402,F401
from vg_descriptor import decode_gam_stream, load_gfa_segments                   # noqa: E402

pytestmark = pytest.mark.gpu

CORRECTED = ("corrected", "corrected_clipped")
NO_CHAINING_ALL = dict(colinear_chaining=False, selection_method=gm.ALL)


class Setup:
    """A graph on the device with its seeder and the letters of its segments, made once per graph."""

    def __init__(self, gca, gfa):   # noqa: F811
        self.gca, self.gfa = gca, gfa
        self.graph = gca.AlignmentGraph(gfa)
        self.seeder = gca.MinimizerSeeder(self.graph)
        self.segments = gfa_segments(gfa)                  # by name
        self.by_id = load_gfa_segments(gfa)               # by the aligner's node id

    def aligner(self, seeded=False, **kw):
        return self.gca.Aligner(self.graph, None if seeded else self.seeder, long_pass=True, chain_traces=1, **kw)


def split(text, off):
    return [text[int(off[k]):int(off[k + 1])] for k in range(len(off) - 1)]


def final_traces(kept, r):
    """(node, offset, seqpos) lists of read r's final alignments (any order): the chained alignment when it won, else the selected whole-read alignments."""
    if kept["chained_better"][r]:
        t = [(int(kept["read_chain_trace_off"][r]), int(kept["read_chain_trace_off"][r + 1]), "chain_trace_")]
    else:
        base = int(kept["read_longall_off"][r])
        t = [(int(kept["long_trace_off"][base + int(k)]), int(kept["long_trace_off"][base + int(k) + 1]), "long_trace_")
             for k in kept["long_index"][int(kept["read_long_off"][r]):int(kept["read_long_off"][r + 1])]]
    return [list(zip(kept[p + "node"][a:b].tolist(), kept[p + "offset"][a:b].tolist(), kept[p + "seqpos"][a:b].tolist())) for a, b, p in t]


def spell_cells_on_path(line, cells, setup):
    """The letters of a GAF line's path under the cells of a trace, or None when the trace is not one of this line. Every cell is placed on the path - its node must
    be the step's segment in the step's direction (numbered by first appearance in the GFA), its offset inside it - and a cell that stands where the one before it
    stands adds nothing. Returns (letters, jumps): jumps counts the cells more than one path base behind their predecessor. The reference's backtrace can leave the
    inside of a deletion run out (tests/test_corrected_model.py's tier c, read 1: 19 bases of one node at one read position); AddCorrected spells cells, so the piece
    lacks those bases while the GAF line's path has them."""
    f = line.split(b"\t")
    steps = re.findall(rb"[<>][^<>]+", f[5])
    seqs = [setup.segments[s[1:].decode()] if s[:1] == b">" else setup.segments[s[1:].decode()].translate(COMPLEMENT)[::-1] for s in steps]
    begin = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).tolist()
    if (cells[0][2], cells[-1][2] + 1) != (int(f[2]), int(f[3])):
        return None
    k, coords = 0, []
    for i, (node, offset, _) in enumerate(cells):
        k += i > 0 and node != cells[i - 1][0]
        if k >= len(steps) or (node & 1) != (steps[k][:1] == b"<") or setup.by_id[node >> 1].encode() != setup.segments[steps[k][1:].decode()] or offset >= len(seqs[k]):
            return None
        coords.append(begin[k] + offset)
    if k != len(steps) - 1 or coords[0] != int(f[7]) or coords[-1] + 1 != int(f[8]):
        return None
    path = b"".join(seqs)
    return bytes(path[c] for i, c in enumerate(coords) if i == 0 or c != coords[i - 1]), sum(b < a or b > a + 1 for a, b in zip(coords, coords[1:]))


def mode_case(setup, reads, names, std_sort, hits=None, **mode):   # noqa: F811
    """One batch three ways - device_output 1 | 8, 8 alone, kept traces without the bit through format_batch - under the mode's keyword arguments. Asserts (i) both
    record files of the three runs are byte-equal, (ii) they are corrected_model.batch_records over the kept traces in the replayed order, (iii) every clipped record's
    piece is the path of its GAF line between path start and end - or, where a trace leaves part of a deletion run out, the path's letters under that trace's cells
    (spell_cells_on_path) - and its header carries that line's read start and end, (iv) one record per read that is not flagged. hits: caller-supplied seed
    hits per read (the seeded entry point). Returns the three results and what the cases look at."""
    gca, graph = setup.gca, setup.graph   # noqa: F811
    batch = gca.ReadBatch(reads)
    seeds = {} if hits is None else {"seeds": gca.SeedBatch(graph, batch, hits)}
    host = setup.aligner(seeded=hits is not None, keep_traces=True, **mode)
    kept = host.align_batch(batch, **seeds)
    texts, _ = host.format_batch(kept, batch, names, formats=CORRECTED)
    dev = setup.aligner(seeded=hits is not None, device_output=1 | 8, **mode).align_batch(batch, gaf_names=names, formats=("gaf",) + CORRECTED, **seeds)
    alone = setup.aligner(seeded=hits is not None, device_output=8, **mode).align_batch(batch, gaf_names=names, formats=CORRECTED, **seeds)
    # (i)
    for fmt in CORRECTED:
        assert dev[fmt] == texts[fmt], fmt
        assert alone[fmt] == dev[fmt], fmt
        assert int(dev[fmt + "_rec_off"][-1]) == len(dev[fmt])
    assert int(alone["out_path_off"][-1]) == 0 and int(alone["out_vg_off"][-1]) == 0
    # (ii)
    want_bodies, want_clipped = cm.batch_records(kept, names, reads, letter_of(gca, graph, kept), std_sort)
    bodies, clipped = split(dev["corrected"], dev["corrected_rec_off"]), split(dev["corrected_clipped"], dev["corrected_clipped_rec_off"])
    assert clipped == want_clipped
    assert bodies == want_bodies
    # (iii): against the device's own GAF lines, not against the model's records
    lines = dev["gaf"].splitlines()
    assert len(lines) == len(clipped)
    index_in_read, last, with_jumps, unused = [], None, 0, []
    for line, record in zip(lines, clipped):
        f = line.split(b"\t")
        if f[0] != last:
            unused = final_traces(kept, names.index(f[0]))
        index_in_read.append(index_in_read[-1] + 1 if f[0] == last else 0)
        last = f[0]
        header, piece, rest = record.split(b"\n")
        assert rest == b"" and header == b">" + f[0] + b"_%d_" % index_in_read[-1] + f[2] + b"_" + f[3]
        if piece == spell_gaf_line(line, setup.segments):
            continue
        # not the whole path: then one of the read's traces lies on this line's path, leaves part of a deletion run out, and the piece is the path's letters under its cells
        on_path = [spell_cells_on_path(line, t, setup) for t in unused]
        explained = [k for k, spelled in enumerate(on_path) if spelled is not None and spelled[1] > 0 and spelled[0] == piece]
        assert explained, header
        del unused[explained[0]]
        with_jumps += 1
    # (iv)
    flagged = (np.asarray(kept["failed_assertion"]) != 0) | (np.asarray(kept["capacity_exceeded"]) != 0)
    assert len(bodies) == len(reads) - int(flagged.sum())
    assert [b.split(b"\n")[0][1:] for b in bodies] == [n for n, f in zip(names, flagged) if not f]
    return {"kept": kept, "dev": dev, "alone": alone, "bodies": bodies, "clipped": clipped, "lines": lines, "flagged": flagged, "lines with a skipped run": with_jumps,
            "winners": [r for r in range(len(reads)) if kept["chained_better"][r] and not flagged[r]], "records per read": np.diff(np.asarray(dev["read_out_off"]).astype(np.int64))}


def names_of(reads, prefix=b"r"):
    return [prefix + b"%d" % i for i in range(len(reads))]


# ---------------------------------------------------------------- 1. without chaining, 7. the seeded entry

@pytest.fixture(scope="module")
def ga_setup(gca, ga_inputs):   # noqa: F811
    return Setup(gca, ga_inputs.gfa)


@pytest.mark.parametrize("method", [gm.GREEDY_LENGTH, gm.ALL, gm.SCHEDULE_SCORE])
def test_without_chaining(ga_setup, ga_inputs, std_sort, method):   # noqa: F811
    reads = ga_inputs.reads
    seen = mode_case(ga_setup, reads, names_of(reads), std_sort, colinear_chaining=False, selection_method=method)
    assert seen["winners"] == [] and not np.any(seen["kept"]["chained_better"])
    print("records per read:", seen["records per read"].tolist())
    assert len(seen["bodies"]) == len(reads)
    if method == gm.ALL:
        assert int(np.sum(seen["records per read"] >= 2)) >= 1
        overlapping = sum(int(a.split(b"\t")[0] == b.split(b"\t")[0] and int(b.split(b"\t")[2]) < int(a.split(b"\t")[3])) for a, b in zip(seen["lines"], seen["lines"][1:]))
        print("lines that start before their predecessor's end:", overlapping)


def test_the_seeded_entry(ga_setup, ga_inputs, std_sort):   # noqa: F811
    """gc_align_batch_seeded with the bit set: with the seeding model's hits (which tests/test_seed_hits_gpu.py holds to the minimizer seeder's) the records are those of
    the minimizer-seeded run, with chaining and without."""
    reads = ga_inputs.reads
    names = names_of(reads)
    hits = [[(s["nodeID"], s["nodeOffset"], s["seqPos"], s["matchLen"], s["raw"], int(s["reverse"]))
             for s in seeding_model.get_seeds(read, ga_inputs.index, ga_inputs.graph, 15, 20, 10.0, std_sort)] for read in reads]
    assert sum(len(h) for h in hits) > 100
    for mode in ({}, NO_CHAINING_ALL):
        own = mode_case(ga_setup, reads, names, std_sort, **mode)
        seeded = mode_case(ga_setup, reads, names, std_sort, hits=hits, **mode)
        for fmt in CORRECTED + ("gaf",):
            assert seeded["dev"][fmt] == own["dev"][fmt], (mode, fmt)
        assert len(own["clipped"]) >= len(reads)


# ---------------------------------------------------------------- 2. the order through tied starts, 8. buffers reused

class TiedInputs:
    """tests/lowcomplexity.py's tier c, reads 1 to 5, and tier a, reads 3 and 6, each on its own graph: reads inside tandem arrays, with tens of whole-read alignments
    that share their starts (tests/test_corrected_model.py shows it with the oracle)."""

    def __init__(self, gca, directory):   # noqa: F811
        self.sets = {}
        for tier, picked in (("c", [1, 2, 3, 4, 5]), ("a", [3, 6])):
            g, reads, _ = lc.tier(tier)
            gfa = os.path.join(str(directory), tier + ".gfa")
            g.write_gfa(gfa)
            self.sets[tier] = (Setup(gca, gfa), [reads[i] for i in picked], [b"%s%d" % (tier.encode(), i) for i in picked])


@pytest.fixture(scope="module")
def tied(gca, tmp_path_factory):   # noqa: F811
    return TiedInputs(gca, tmp_path_factory.mktemp("tied"))


def test_the_order_through_tied_starts(tied, std_sort):   # noqa: F811
    """More than 16 selected alignments per read with tied starts: the lines of every writer come in the order of std::sort applied twice to the selection's order,
    which is neither the stable order nor the order after one sort."""
    twice_not_stable = once_not_twice = backwards = 0
    for tier, (setup, reads, names) in tied.sets.items():
        gca = setup.gca   # noqa: F811
        seen = mode_case(setup, reads, names, std_sort, **NO_CHAINING_ALL)
        kept = seen["kept"]
        assert not seen["flagged"].any() and seen["winners"] == []
        want = []
        for r in range(len(reads)):
            base = int(kept["read_longall_off"][r])
            alns = [base + int(k) for k in kept["long_index"][int(kept["read_long_off"][r]):int(kept["read_long_off"][r + 1])]]
            starts, ends = [int(kept["longall_start"][a]) for a in alns], [int(kept["longall_end"][a]) for a in alns]
            shape = tie_shape(starts, ends, std_sort)
            print(tier, names[r], "(alignments, tied starts, twice != stable, once != stable, once != twice, ends moving backwards)", shape)
            twice_not_stable += shape[0] > 16 and shape[2]
            once_not_twice += shape[0] > 16 and shape[4]
            backwards += shape[5] > 0
            want += [(names[r], starts[i], ends[i]) for i in cm.output_order(starts, std_sort)]
        print(tier, "lines whose trace leaves part of a deletion run out:", seen["lines with a skipped run"], "of", len(seen["lines"]))
        # every GAF line in the model's order, line by line
        got = [(f[0], int(f[2]), int(f[3])) for f in (line.split(b"\t") for line in seen["lines"])]
        assert got == want
        # the device's encoders and the host's over kept traces: the same GAF, JSON and GAM, one line and one message per alignment
        batch = gca.ReadBatch(reads)
        dev = setup.aligner(device_output=1 | 4 | 8, **NO_CHAINING_ALL).align_batch(batch, gaf_names=names, other_formats=True)
        host = setup.aligner(keep_traces=True, **NO_CHAINING_ALL).align_batch(batch, gaf_names=names, other_formats=True)
        assert dev["gaf"] == host["gaf"] == seen["dev"]["gaf"] and dev["gaf_chained_skipped"] == 0
        assert dev["json"] == host["json"]
        inflated = gzip.decompress(dev["gam"])
        assert inflated == gzip.decompress(host["gam"])
        assert dev["json"].count(b"\n") == len(want)
        assert sum(len(group) for group in decode_gam_stream(inflated)) == len(want)
    assert twice_not_stable >= 3 and once_not_twice >= 2 and backwards >= 1, (twice_not_stable, once_not_twice, backwards)


def test_the_streams_buffers_reused_by_calls_of_other_sizes(tied):
    """One aligner (one stream: corrLens, corrOffsets, corrText and their pinned twins) with device_output = 8: a batch with hundreds of pieces, one with a single
    piece, the first again; then three aligners with the three batches in flight on one device."""
    from graphchainer_amd.workqueue import ReadQueue, run_queue
    setup, reads, names = tied.sets["c"]
    gca = setup.gca   # noqa: F811
    rng = np.random.default_rng(19)
    short = [reads[0][300:800], bytes(rng.choice(list(b"ACGT"), size=500).tolist())]
    calls = [(reads, names), (short, [b"short", b"random"]), (reads, names)]
    batches = [gca.ReadBatch(r) for r, _ in calls]
    kw = dict(device_output=8, **NO_CHAINING_ALL)

    def run(aligner, k):
        out = aligner.align_batch(batches[k], gaf_names=calls[k][1], formats=CORRECTED)
        return {fmt: out[fmt] for fmt in CORRECTED}, np.diff(np.asarray(out["read_out_off"]).astype(np.int64)).tolist()
    one = setup.aligner(**kw)
    serial = [run(one, k) for k in range(3)]
    print("pieces per read:", [s[1] for s in serial], "bytes:", [len(s[0]["corrected_clipped"]) for s in serial])
    assert serial[0] == serial[2]
    assert serial[1] == run(setup.aligner(**kw), 1)
    assert serial[1][1][0] >= 1 and serial[1][1][1] == 0 and sum(serial[0][1]) > 100                  # the second call is far smaller, one of its reads has no alignment
    assert serial[1][0]["corrected"].endswith(b">random\n" + short[1].lower() + b"\n")
    aligners = [setup.aligner(**kw) for _ in range(3)]
    for _ in range(2):                                                                                  # (the second pass finds every stream's buffers used)
        parts = run_queue(ReadQueue(3), lambda worker, k: run(aligners[worker], k), workers=3)
        assert sorted(k for k, _ in parts) == [0, 1, 2]
        for k, got in parts:
            assert got == serial[k], k


# ---------------------------------------------------------------- 3. fast mode

def test_fast_mode(gca, tmp_path, std_sort):   # noqa: F811
    """A chained winner's trace comes from k_fast_chain_trace: its piece is the letters of the stitched piece, one per path base, under chain_aln_start / chain_aln_end."""
    from graphchainer_amd.synth import SynthGraph
    sg = SynthGraph(40_000, seed=23, repeats=3)
    gfa = str(tmp_path / "g.gfa")
    sg.write_gfa(gfa)
    reads = make_reads(sg)[0]
    names = names_of(reads)
    setup = Setup(gca, gfa)
    seen = mode_case(setup, reads, names, std_sort, fast_mode=True, colinear_gap=GAP)
    kept, winners = seen["kept"], seen["winners"]
    print("chained winners:", winners)
    assert len(winners) >= 2
    graph = setup.graph
    length, ids, offset = graph.array("nodeLength"), graph.array("nodeIDs"), graph.array("nodeOffset")
    records = {}
    for record in seen["clipped"]:
        records.setdefault(record.split(b"_")[0][1:], []).append(record)
    for r in winners:
        path = [int(v) for v in kept["path_node"][int(kept["read_path_off"][r]):int(kept["read_path_off"][r + 1])]]
        cells = path_to_trace(path, int(kept["path_first_offset"][r]), int(kept["path_last_offset"][r]), length)
        assert len(cells) == int(kept["path_cells"][r])
        piece = gca.api.graph_letters(graph, [int(ids[v]) for v, _ in cells], [o + int(offset[v]) for v, o in cells])
        assert records[names[r]] == [b">" + names[r] + b"_0_%d_%d\n" % (int(kept["chain_aln_start"][r]), int(kept["chain_aln_end"][r])) + piece + b"\n"], names[r]


# ---------------------------------------------------------------- 4. forced global, 5. clipping, 6. the band controls

@pytest.fixture(scope="module")
def whole(gca, tmp_path_factory):   # noqa: F811
    inputs = Inputs(tmp_path_factory.mktemp("whole"))
    setup = Setup(gca, inputs.gfa)
    setup.backbone = inputs.bb
    return setup, inputs.whole


def end_run(values):
    """Length of the longer of the runs of equal values at the two ends of a list."""
    head = next((i for i, v in enumerate(values) if v != values[0]), len(values))
    tail = next((i for i, v in enumerate(reversed(values)) if v != values[-1]), len(values))
    return max(head, tail)


def longest_run(values):
    best = run = 0
    for i, v in enumerate(values):
        run = run + 1 if i and v == values[i - 1] else 1
        best = max(best, run)
    return best


def test_forced_global(whole, std_sort):   # noqa: F811
    """Alignments that reach both ends of the read however poor: insertion runs (one graph position, nothing spelled) and deletion runs (one read position, every
    letter spelled) at the ends of a trace."""
    setup, reads = whole
    # On the shared reads alone the final alignments' longest runs are 2 cells on one graph position and 5 on one read position (measured on an MI355X): their junk
    # is aligned against graph that goes on. Four more reads from the same backbone bring the runs: junk beyond either end of the graph, and deletions of 12 and 30 bases.
    bb, rng = setup.backbone, np.random.default_rng(29)
    junk = lambda n: bytes(rng.choice(list(b"ACGT"), size=n).tolist())   # noqa: E731
    reads = reads + [bb[-300:] + junk(120), junk(120) + bb[:300], bb[6000:6300] + bb[6312:6600], bb[8000:8300] + bb[8330:8600]]
    seen = mode_case(setup, reads, names_of(reads), std_sort, force_global=True)
    traces = [t for r in range(len(reads)) if not seen["flagged"][r] for t in final_traces(seen["kept"], r)]
    on_graph = [end_run([(c[0], c[1]) for c in t]) for t in traces]
    on_read = [longest_run([c[2] for c in t]) for t in traces]
    print("cells on one graph position at a trace's end:", on_graph, "longest run on one read position:", on_read, "winners", seen["winners"])
    assert max(on_graph) >= 10 and max(on_read) >= 10


@pytest.mark.parametrize("x_drop", [0, 50])
def test_clipping(gca, tmp_path, std_sort, x_drop):   # noqa: F811
    """Alignments that end mid-read: behind the last one the corrected record is the read's own letters, lower-cased."""
    inputs = ClipInputs(tmp_path)
    setup, reads = Setup(gca, inputs.gfa), inputs.whole
    names = names_of(reads)
    seen = mode_case(setup, reads, names, std_sort, precise_clipping=0.66, x_drop=x_drop)
    last = {}
    for line in seen["lines"]:
        f = line.split(b"\t")
        last[f[0]] = (int(f[1]), int(f[3]))                                   # the read's last line in output order: where currentEnd is left
    mid_read = sum(int(f[3]) < int(f[1]) for f in (line.split(b"\t") for line in seen["lines"]))
    tails = 0
    for body in seen["bodies"]:
        name, text = body.split(b"\n")[:2]
        r = names.index(name[1:])
        if name[1:] not in last:
            assert text == reads[r].lower()
            continue
        length, end = last[name[1:]]
        assert length == len(reads[r])
        assert text[len(text) - (length - end):] == reads[r][end:].lower()
        assert end == 0 or text[:len(text) - (length - end)][-1:].isupper()      # ... and in front of it stands the last piece, in upper case
        tails += end < length
    print("lines ending before the read's end:", mid_read, "records with a raw tail:", tails)
    assert mid_read >= 2 and tails >= 2


def test_the_band_controls(whole, std_sort):   # noqa: F811
    """The ramp, and a cell limit that is reached: chosen from the unlimited run's own traces - a slice computes at least the columns its alignment crosses in it, and
    the limit is the lower quartile of those counts, so three quarters of these slices alone reach it. That it is reached shows in the work the two runs report: a
    limit that no slice reaches leaves every count as it was (measured on an MI355X: 47 848 column steps without, 73 108 with the limit of 60, 12 and 17 records -
    alignments that break off leave more seeds to extend)."""
    setup, reads = whole
    names = names_of(reads)
    mode_case(setup, reads, names, std_sort, ramp_bandwidth=25)
    unlimited = mode_case(setup, reads, names, std_sort)
    columns = []
    for r in range(len(reads)):
        for t in final_traces(unlimited["kept"], r):
            per_slice = {}
            for node, offset, seqpos in t:
                per_slice.setdefault(seqpos // 64, set()).add((node, offset))
            columns += [len(c) for c in per_slice.values()]
    limit = sorted(columns)[len(columns) // 4]
    limited = mode_case(setup, reads, names, std_sort, max_cells_per_slice=limit)
    steps = int(unlimited["kept"]["counters_long"][2]), int(limited["kept"]["counters_long"][2])
    print("limit", limit, "of", len(columns), "slices; column steps of the whole-read pass without and with it:", steps, "records", len(unlimited["clipped"]), len(limited["clipped"]))
    assert sum(c >= limit for c in columns) >= 3 * len(columns) // 4 and steps[1] != steps[0]
    assert not np.array_equal(np.asarray(unlimited["kept"]["longall_end"]), np.asarray(limited["kept"]["longall_end"]))
    assert len(limited["clipped"]) >= 1
