"""Corrected reads on the device (gc_params::device_output & 8; hip/gc_corrected.hip): the kernels on traces of exact shapes (gc_corrected_pieces), a batch against
tests/corrected_model.py over the traces of a keep_traces run and, independently of any model, against the letters of each GAF line's path, and the bit left clear."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import corrected_model as cm                                                     # noqa: E402
from test_corrected_host import KEPT_REPEATS, LENGTHS, VARIANTS                  # noqa: E402
from test_gpu_parity import gca                                                  # noqa: E402,F401

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden")


# ---------------------------------------------------------------- the kernels on exact shapes

@pytest.fixture(scope="module")
def iupac_world(gca, tmp_path_factory):   # noqa: F811
    """tests/letters_inputs.py's IUPAC graph on the device, and a tape of its cells: split nodes with a letter outside ACGT and plain ones in turn, each node's last
    cell flagged nodeSwitch. (The kernels look at cells, not at edges: consecutive tape nodes need not be neighbours.)"""
    from letters_inputs import LettersInputs
    inputs = LettersInputs(tmp_path_factory.mktemp("corrected_letters"))
    graph = gca.AlignmentGraph(inputs.gfa)
    ids, off, length = graph.array("nodeIDs"), graph.array("nodeOffset"), graph.array("nodeLength")
    first_ambiguous = None
    cells_of = lambda v: [(int(ids[v]), int(off[v]) + o) for o in range(int(length[v]))]   # noqa: E731
    n = len(ids)
    tail = [c for v in range(n - 400, n) for c in cells_of(v)]                  # (ambiguous split nodes are numbered last: src/AlignmentGraph.cpp:255-307)
    text = gca.api.graph_letters(graph, [c[0] for c in tail], [c[1] for c in tail])
    at, ambiguous = 0, []
    for v in range(n - 400, n):
        if any(chr(c) not in "ACGT" for c in text[at:at + int(length[v])]):
            ambiguous.append(v)
        at += int(length[v])
    assert len(ambiguous) >= 20
    tape = []
    for k, v in enumerate(ambiguous[:20]):
        for w in (v, 50 + 7 * k):
            cells = [(a, b, 0) for a, b in cells_of(w)]
            cells[-1] = (cells[-1][0], cells[-1][1], 1)
            tape += cells
    letters = gca.api.graph_letters(graph, [c[0] for c in tape], [c[1] for c in tape])
    table = {(c[0], c[1]): letters[i:i + 1] for i, c in enumerate(tape)}
    assert len(tape) >= 400 and any(chr(c) not in "ACGT" for c in letters[:200])
    return graph, tape, (lambda node, offset: table[(node, offset)])


def tape_trace(tape, start, n, repeats, flagged_before=()):
    """n cells along the tape from `start`: a cell in `repeats` stands where the one before it does, every other is the tape's next cell (with its nodeSwitch flag)."""
    cells, at = [], start
    for i in range(n):
        if i > 0 and i not in repeats:
            at += 1
        node, offset, switch = tape[at]
        if i + 1 in repeats and i + 1 < n:
            switch = 1 if (i + 1) in flagged_before else 0                       # the next cell repeats this one: an insertion unless this cell is flagged
        cells.append((node, offset, switch))
    return cells


def shapes(tape):
    out = []
    for k, n in enumerate(LENGTHS):
        for name, repeats in VARIANTS.items():
            out.append(tape_trace(tape, 3 * k, n, {i for i in repeats(n) if i < n}))
        out.append(tape_trace(tape, 3 * k, n, {i for i in KEPT_REPEATS if i < n}, flagged_before=KEPT_REPEATS))
    return out


def as_arrays(trace):
    return [c[0] for c in trace], [c[1] for c in trace], [c[2] for c in trace]


def test_pieces_on_exact_shapes(gca, iupac_world):   # noqa: F811
    graph, tape, letter = iupac_world
    traces = shapes(tape)
    assert len(traces) == 64 and {len(t) for t in traces} == set(LENGTHS)
    want = [cm.add_corrected(t, letter) for t in traces]
    assert any(len(w) < len(t) for w, t in zip(want, traces)) and any(set(w) - set(b"ACGT") for w in want)
    one_cell = [tape[5]]
    calls = {
        "no alignment": [],
        "one alignment of one cell": [one_cell],
        "64 alignments": traces,
        "65 alignments": traces + [one_cell],
        "3075 alignments: three jobs per thread of the scan's block": (traces[:41] + [one_cell]) * 73 + traces[:9],
    }
    assert len(calls["3075 alignments: three jobs per thread of the scan's block"]) == 3075
    for name, call in calls.items():
        got = gca.api.corrected_pieces(graph, [as_arrays(t) for t in call])
        assert got == [cm.add_corrected(t, letter) for t in call], name
    # the host's spelling of one trace is the same function
    for t in traces[::7]:
        assert gca.api.format_corrected_trace(graph, *as_arrays(t)) == cm.add_corrected(t, letter)
    # cells outside the graph are refused before anything is launched
    with pytest.raises(RuntimeError):
        gca.api.corrected_pieces(graph, [([tape[0][0]], [1 << 30], [0])])
    with pytest.raises(RuntimeError):
        gca.api.corrected_pieces(graph, [([-5], [0], [0])])


# ---------------------------------------------------------------- a batch

COMPLEMENT = bytes.maketrans(b"ACGTRYKMSWBDHVN", b"TGCAYRMKSWVHDBN")


def gfa_segments(gfa):
    """name -> sequence, held to vg_descriptor.load_gfa_segments (which numbers the segments by first appearance)."""
    from vg_descriptor import load_gfa_segments
    by_name = {}
    for line in open(gfa):
        if line[0] == "S":
            name, seq = line[1:].strip().split()[:2]
            by_name[name] = seq.encode()
    by_id = load_gfa_segments(gfa)
    assert sorted(s.encode() for s in by_id.values()) == sorted(by_name.values())
    return by_name


def spell_gaf_line(line, segments):
    """The letters of a GAF line's path between its columns 8 and 9 (path start and end)."""
    f = line.split(b"\t")
    path = b""
    for step in re.findall(rb"[<>][^<>]+", f[5]):
        seq = segments[step[1:].decode()]
        path += seq if step[:1] == b">" else seq.translate(COMPLEMENT)[::-1]
    assert len(path) == int(f[6])
    return path[int(f[7]):int(f[8])]


def letter_of(gca, graph, out):   # noqa: F811
    """TraceItem::graphCharacter for every cell of the result's kept traces (gc_graph_letters, which tests/test_letters_gpu.py holds to the model's graph)."""
    table = {}
    for nodes, offsets in ((out["long_trace_node"], out["long_trace_offset"]), (out["chain_trace_node"], out["chain_trace_offset"])):
        if len(nodes):
            text = gca.api.graph_letters(graph, nodes, offsets)
            table.update(zip(zip(np.asarray(nodes).tolist(), np.asarray(offsets).tolist()), (text[i:i + 1] for i in range(len(text)))))
    return lambda node, offset: table[(node, offset)]


def batch_case(gca, gfa, reads, names):   # noqa: F811
    graph = gca.AlignmentGraph(gfa)
    seeder = gca.MinimizerSeeder(graph)
    batch = gca.ReadBatch(reads)
    kept = gca.Aligner(graph, seeder, long_pass=True, keep_traces=True, chain_traces=1).align_batch(batch)
    aligner = gca.Aligner(graph, seeder, long_pass=True, chain_traces=1, device_output=1 | 8)
    dev = aligner.align_batch(batch, gaf_names=names, formats=("gaf", "corrected", "corrected_clipped"))
    want_bodies, want_clipped = cm.batch_records(kept, names, reads, letter_of(gca, graph, kept))
    split = lambda text, off: [text[int(off[k]):int(off[k + 1])] for k in range(len(off) - 1)]   # noqa: E731
    assert int(dev["corrected_rec_off"][-1]) == len(dev["corrected"]) and int(dev["corrected_clipped_rec_off"][-1]) == len(dev["corrected_clipped"])
    assert split(dev["corrected"], dev["corrected_rec_off"]) == want_bodies
    assert split(dev["corrected_clipped"], dev["corrected_clipped_rec_off"]) == want_clipped
    # the host's spelling from the kept traces, without the bit: the same records
    host = gca.Aligner(graph, seeder, long_pass=True, keep_traces=True, chain_traces=1)
    texts, _ = host.format_batch(kept, batch, names, formats=("corrected", "corrected_clipped"))
    assert texts["corrected"] == dev["corrected"] and texts["corrected_clipped"] == dev["corrected_clipped"]
    # independently of any model: every piece is the path of its GAF line between the path's start and end
    segments = gfa_segments(gfa)
    lines = dev["gaf"].splitlines()
    assert len(lines) == len(want_clipped)
    for line, record in zip(lines, want_clipped):
        header, piece = record.split(b"\n")[:2]
        f = line.split(b"\t")
        assert header == b">" + f[0] + b"_" + header.split(b"_")[-3] + b"_" + f[2] + b"_" + f[3]      # read name, read start and end
        assert piece == spell_gaf_line(line, segments)
    # bit 8 alone: the same records, no GAF or vg pieces
    alone = gca.Aligner(graph, seeder, long_pass=True, chain_traces=1, device_output=8).align_batch(batch, gaf_names=names, formats=("corrected", "corrected_clipped"))
    assert alone["corrected"] == dev["corrected"] and alone["corrected_clipped"] == dev["corrected_clipped"]
    assert int(alone["out_path_off"][-1]) == 0 and int(alone["out_vg_off"][-1]) == 0 and int(alone["out_corrected_off"][-1]) > 0
    n_out = np.diff(np.asarray(dev["read_out_off"]).astype(np.int64))
    flagged = (np.asarray(kept["failed_assertion"]) != 0) | (np.asarray(kept["capacity_exceeded"]) != 0)
    return {"chained winners": int(np.sum(np.asarray(kept["chained_better"]) != 0)), "reads with two or more alignments": int(np.sum(n_out >= 2)),
            "reads without alignments": int(np.sum((n_out == 0) & ~flagged)), "flagged reads": int(np.sum(flagged)), "records": len(want_bodies), "reads": len(reads)}


def test_batch_against_model_and_path(gca, tmp_path):   # noqa: F811
    from graphchainer_amd.synth import SynthGraph
    reads = [l.strip().encode() for l in open(os.path.join(GOLD, "syn20k.fa")) if not l.startswith(">")]
    seen = [batch_case(gca, os.path.join(GOLD, "syn20k.gfa"), reads, [b"r%d" % i for i in range(len(reads))])]
    sg = SynthGraph(300_000, seed=17, repeats=3, repeat_len=1500)
    gfa = str(tmp_path / "g.gfa")
    sg.write_gfa(gfa)
    reads = sg.sample_reads(160, 3000, seed=77, sv_fraction=0.3, sv_len=600)
    reads[3] = reads[3].lower()                                               # lower case in the read: the raw stretches stay lower case, the alignment is the same
    reads.insert(7, b"A" * 1500)                                              # no minimizer of a homopolymer is in the graph: no alignment, its lower-cased self
    reads.insert(20, reads[20][:700] + b"X" + reads[20][701:])                # a letter outside the alphabet: flagged, no record
    names = [b"read%d some description" % i for i in range(len(reads))]       # the id is the whole line: not cut at white space
    seen.append(batch_case(gca, gfa, reads, names))
    print(seen)
    total = {k: sum(s[k] for s in seen) for k in seen[0]}
    assert total["chained winners"] >= 1 and total["reads with two or more alignments"] >= 1 and total["reads without alignments"] >= 1 and total["flagged reads"] >= 1
    assert total["records"] == total["reads"] - total["flagged reads"]       # no read is left out


def test_bit_clear_changes_nothing(gca):   # noqa: F811
    """device_output = 1 | 4: the GAF and JSON text are the files recorded before the corrected reads existed, every array of the result equals the run with the bit
    set (which only adds to it), and the two new pointers are NULL."""
    gfa = os.path.join(GOLD, "syn20k.gfa")
    reads = [l.strip().encode() for l in open(os.path.join(GOLD, "syn20k.fa")) if not l.startswith(">")]
    names = [b"r%d" % i for i in range(len(reads))]
    graph = gca.AlignmentGraph(gfa)
    seeder = gca.MinimizerSeeder(graph)
    batch = gca.ReadBatch(reads)
    clear = gca.Aligner(graph, seeder, long_pass=True, device_output=1 | 4).align_batch(batch, gaf_names=names, formats=("gaf", "json"))
    res = clear._holder.res.contents
    assert not res.out_corrected_off and not res.out_corrected_text and res.device_output == 5
    assert "out_corrected_off" not in clear
    assert clear["gaf"] == open(os.path.join(GOLD, "syn20k.expected.gaf"), "rb").read()
    assert clear["json"] == open(os.path.join(GOLD, "syn20k.expected.json"), "rb").read()
    with_bit = gca.Aligner(graph, seeder, long_pass=True, device_output=1 | 4 | 8).align_batch(batch, gaf_names=names, formats=("gaf", "json"))
    assert bool(with_bit._holder.res.contents.out_corrected_off) and "out_corrected_off" in with_bit
    timing = {"kernel_us", "host_us"}
    assert set(clear) == set(with_bit) - {"out_corrected_off"}
    for key in clear:
        if key in timing:
            continue
        a, b = clear[key], with_bit[key]
        assert (a == b) if isinstance(a, bytes) else np.array_equal(np.asarray(a), np.asarray(b)), key
    for res_ in (clear, with_bit):
        n_out = int(res_["read_out_off"][-1])
        r = res_._holder.res.contents
        assert res_["gaf"].count(b"\n") == n_out
        assert bytes(r.out_path_text[:int(res_["out_path_off"][-1])]) == bytes(with_bit._holder.res.contents.out_path_text[:int(with_bit["out_path_off"][-1])])
    with pytest.raises(RuntimeError):                                         # a result without the pieces and without kept traces cannot give the records
        gca.Aligner(graph, seeder, long_pass=True, device_output=1 | 4).format_batch(clear, batch, names, formats=("corrected",))
