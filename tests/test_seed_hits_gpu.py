"""Caller-supplied seed hits (gc_seeds_upload + gc_align_batch_seeded; SeedBatch / Aligner.align_batch(seeds=...)) on the GPU:
  1. the minimizer model's own hits, handed over as foreign seeds, give the oracle's result array for array (and leave the aligner's minimizer path as it was);
  2. hits the minimizer path cannot produce - thinned, shuffled, matchLen 2..60 per hit, hits on the read's first and last base, in a segment's short last split node, duplicates,
     a read without hits, reads the reference asserts on - against the Python models alone (tests/seeding_model.py, tests/alignment_model.py);
  3. hits a kernel would read out of bounds through are refused at upload, by name, before anything reads through them."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import seeding_model                                        # noqa: E402
from graphchainer_amd.synth import SynthGraph              # noqa: E402  (test inputs)
from test_alignment_model import _models                    # noqa: E402
from test_gpu_parity import COMPARE_KEYS, LONG_KEYS, compare, expand_stitched_path, gca, mark_missing_chain_alignments   # noqa: E402,F401  (gca: the fixture)
from test_seeding_model import _inputs, std_sort            # noqa: E402,F401  (the fixture)

pytestmark = pytest.mark.gpu

_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _as_hit(s):
    return (s["nodeID"], s["nodeOffset"], s["seqPos"], s["matchLen"], s["raw"], int(s["reverse"]))


def _normalised(out, graph):
    """What test_gpu_parity.run_case does with a result before it compares it with the oracle's."""
    got = {k: (v.astype(np.int64) if isinstance(v, np.ndarray) and v.dtype.kind in "ui" and k not in ("counters", "counters_long") else v) for k, v in out.items()}
    expand_stitched_path(got, graph.array("nodeLength"))
    mark_missing_chain_alignments(got)
    sel = np.repeat(got["read_longall_off"][:-1], np.diff(got["read_long_off"])) + got["long_index"]
    for key in ("start", "end", "score"):
        got["long_" + key] = got["longall_" + key][sel]
    return got


def _same_seeds_same_result(gca, gfa, reads, std_sort):
    from oracle import Oracle
    oracle = Oracle(gfa, long_pass=True)
    want = oracle.align(reads)
    graph_arrays, index = _inputs(oracle)
    hits = [[_as_hit(s) for s in seeding_model.get_seeds(read, index, graph_arrays, 15, 20, 10.0, std_sort)] for read in reads]
    assert sum(len(h) for h in hits) == int(want["read_seed_off"][-1]) > 0
    graph = gca.AlignmentGraph(gfa)
    batch = gca.ReadBatch(reads)
    seeds = gca.SeedBatch(graph, batch, hits)
    kw = dict(keep_traces=True, keep_seeds=True, long_pass=True, chain_traces=2)
    own = gca.Aligner(graph, None, **kw)                       # a host with its own seeds builds no minimizer index
    compare(_normalised(own.align_batch(batch, seeds=seeds), graph), want, COMPARE_KEYS + LONG_KEYS)
    with pytest.raises(ValueError):
        own.align_batch(batch)
    # structured arrays in place of tuples; an aligner that has a seeder takes the caller's seeds all the same, and its minimizer-seeded run afterwards is what it was
    arrays = [np.array(h, dtype=gca.api.SEED_HIT_DTYPE) for h in hits]
    both = gca.Aligner(graph, gca.MinimizerSeeder(graph), **kw)
    compare(_normalised(both.align_batch(batch, seeds=gca.SeedBatch(graph, batch, arrays)), graph), want, COMPARE_KEYS + LONG_KEYS)
    compare(_normalised(both.align_batch(batch), graph), want, COMPARE_KEYS + LONG_KEYS)
    return want


def test_the_minimizer_hits_as_foreign_seeds_give_the_oracles_result(gca, golden_dir, std_sort):   # noqa: F811
    reads = [l.strip().encode() for l in open(os.path.join(golden_dir, "syn20k.fa")) if not l.startswith(">")]
    assert len(reads) == 6
    _same_seeds_same_result(gca, os.path.join(golden_dir, "syn20k.gfa"), reads, std_sort)


def test_foreign_seeds_reach_the_chained_winner(gca, tmp_path, std_sort):   # noqa: F811
    """The inputs of test_gpu_parity.test_chained_alignment_wins: behind external seeds the chained alignment wins for the deletion reads too (stitching, k_edit_path)."""
    sg = SynthGraph(200_000, seed=19)
    gfa = str(tmp_path / "g.gfa")
    sg.write_gfa(gfa)
    bb = sg.backbone.tobytes()
    reads = [bb[x:x + 3000] + bb[x + 4500:x + 7500] for x in (10_000, 60_000, 120_000)]
    reads += [reads[0].translate(_COMP)[::-1]]
    reads += sg.sample_reads(3, 4000, seed=8)
    want = _same_seeds_same_result(gca, gfa, reads, std_sort)
    assert int(np.sum(want["chained_better"][:4])) >= 3 and int(np.sum(want["chained_better"][4:])) == 0


def foreign_case(tmp_dir, std_sort):   # noqa: F811
    """Inputs and expected values of test 2; everything expected comes from the Python models. Returns (gfa, reads, hits per read, expected per read)."""
    from oracle import Oracle
    sg = SynthGraph(40_000, seed=37)
    gfa = os.path.join(str(tmp_dir), "foreign.gfa")
    sg.write_gfa(gfa)
    oracle = Oracle(gfa, long_pass=False)                       # (its graph and index arrays are the models' inputs; it aligns nothing here)
    graph, index = _inputs(oracle)
    model = _models(oracle, 10)
    base = sg.sample_reads(2, 1200, seed=6, p_del=0.01, p_sub=0.01, p_ins=0.01) + sg.sample_reads(1, 2400, seed=9, p_del=0.01, p_sub=0.01, p_ins=0.01)   # (the long one: more than 64 hits after the thinning)
    reads = [base[0], base[1], base[2], base[0].translate(_COMP)[::-1], base[2][:300], base[2][300:500], base[1][:200]]
    rng = random.Random(5)
    plain = [seeding_model.get_seeds(read, index, graph, 15, 20, 10.0, std_sort) for read in reads]

    def foreign(seeds, keep_every=3):
        out = [dict(s) for s in seeds[::keep_every]]
        rng.shuffle(out)
        for s in out:
            s["matchLen"] = rng.randint(2, 60)
        return out

    def at_cell(cell, match_len, raw):
        node, off, sp, _ = cell
        split = model.g.unitig_node(node, off)
        return {"nodeID": node // 2, "nodeOffset": off, "seqPos": sp, "matchLen": match_len, "raw": raw, "reverse": bool(node & 1), "agNode": split, "agOffset": off - model.g.node_offset[split],
                "goodness": 0, "cluster": 0}

    hits = [foreign(plain[0]), [], foreign(plain[2]), foreign(plain[3]), [], [], []]
    # read 0: hits on its first and last base and in a segment's short last split node (cells of its own whole-read alignment), and a duplicate
    ordered = seeding_model.order_seeds_by_chaining([dict(s) for s in plain[0]], graph, std_sort)
    trace = model.align_one_way(reads[0], ordered, True)[0][0]["trace"]
    by_pos = {c[2]: c for c in trace}
    hits[0] += [at_cell(by_pos[0], 9, 3), at_cell(by_pos[len(reads[0]) - 1], 31, 0)]
    short = [c for c in trace if model.original_size[c[0]] > 64 and model.original_size[c[0]] % 64 and c[1] >= 64 * (model.original_size[c[0]] // 64)]
    assert short, "no cell in a short last split node"
    hits[0].append(at_cell(short[len(short) // 2], 20, 7))
    assert model.g.length[hits[0][-1]["agNode"]] < 64 and model.g.node_offset[hits[0][-1]["agNode"]] > 0
    hits[0].insert(5, dict(hits[0][2]))
    # read 1: more hits than the seed glue keeps in LDS - every hit eight times with eight lengths
    hits[1] = [dict(s, matchLen=rng.randint(2, 60)) for _ in range(8) for s in plain[1]]
    counts = [len(h) for h in hits]
    assert len(hits[1]) > 1024 and len(hits[2]) > 64 and min(len(hits[0]), len(hits[3])) > 32 and {s["reverse"] for s in hits[0]} | {s["reverse"] for s in hits[3]} == {False, True}, counts
    # read 4 has no hits. Reads 5 and 6 are the reference's two assertions: chainApproxPos + offset < seqPos (src/GraphAligner.h:253), matchLen < 2 (:280)
    # (a chain's approximate positions start in the hundreds of thousands, so the read that breaks the first one is that long; it fails in the seed glue and nothing else runs on it)
    first = min(range(len(graph["chainApproxPos"])), key=lambda v: graph["chainApproxPos"][v])
    beyond = graph["chainApproxPos"][first] + 1
    assert beyond < 1_000_000
    reads[5] = bytes(rng.choice(b"ACGT") for _ in range(beyond + 1))
    hits[5] = [{"nodeID": graph["nodeIDs"][first] // 2, "nodeOffset": graph["nodeOffset"][first], "seqPos": beyond, "matchLen": 15, "raw": 1, "reverse": bool(graph["reverse"][first]), "agNode": first, "agOffset": 0,
                "goodness": 0, "cluster": 0}]
    hits[6] = [dict(s) for s in plain[6][:5]]
    hits[6][3]["matchLen"] = 1
    expected = []
    for r, read in enumerate(reads):
        failed = any(s["matchLen"] < 2 or graph["chainApproxPos"][s["agNode"]] + s["agOffset"] < s["seqPos"] for s in hits[r])
        if failed or not hits[r]:
            expected.append({"failed": failed, "seeds": [], "alignments": [], "anchors": []})
            continue
        ordered = seeding_model.order_seeds_by_chaining([dict(s) for s in hits[r]], graph, std_sort)
        alignments, _ = model.align_one_way(read, ordered, True)
        by_position = seeding_model.fragment_order(ordered, std_sort)
        expected.append({"failed": False, "seeds": by_position, "alignments": alignments, "anchors": model.anchors_of_read(read, by_position)})
    return gfa, reads, [[_as_hit(s) for s in h] for h in hits], expected


def test_seeds_the_minimizer_path_cannot_produce(gca, tmp_path, std_sort):   # noqa: F811
    gfa, reads, hits, expected = foreign_case(tmp_path, std_sort)
    graph = gca.AlignmentGraph(gfa)
    batch = gca.ReadBatch(reads)
    got = gca.Aligner(graph, None, keep_traces=True, keep_seeds=True, long_pass=True).align_batch(batch, seeds=gca.SeedBatch(graph, batch, hits))
    assert got["failed_assertion"].tolist() == [int(e["failed"]) for e in expected] == [0, 0, 0, 0, 0, 1, 1]
    alignments = anchors = 0
    for r, e in enumerate(expected):
        s0, s1 = int(got["read_seed_off"][r]), int(got["read_seed_off"][r + 1])
        seeds = [(s["agNode"], s["agOffset"], s["seqPos"], s["goodness"]) for s in e["seeds"]]
        assert list(zip(got["seed_node"][s0:s1].tolist(), got["seed_offset"][s0:s1].tolist(), got["seed_seqpos"][s0:s1].tolist(), got["seed_goodness"][s0:s1].tolist())) == seeds, r
        a0, a1 = int(got["read_longall_off"][r]), int(got["read_longall_off"][r + 1])
        assert a1 - a0 == len(e["alignments"]), (r, a1 - a0, len(e["alignments"]))
        for k, aln in enumerate(e["alignments"]):
            a = a0 + k
            assert (aln["start"], aln["end"], aln["score"]) == (int(got["longall_start"][a]), int(got["longall_end"][a]), int(got["longall_score"][a])), (r, k)
            t0, t1 = int(got["long_trace_off"][a]), int(got["long_trace_off"][a + 1])
            cells = list(zip(got["long_trace_node"][t0:t1].tolist(), got["long_trace_offset"][t0:t1].tolist(), got["long_trace_seqpos"][t0:t1].tolist(), [bool(x) for x in got["long_trace_switch"][t0:t1]]))
            assert [tuple(c) for c in aln["trace"]] == cells, (r, k)
        b0, b1 = int(got["read_anchor_off"][r]), int(got["read_anchor_off"][r + 1])
        assert b1 - b0 == len(e["anchors"]), (r, b1 - b0, len(e["anchors"]))
        for k, (x, y, path, first, last, score) in enumerate(e["anchors"]):
            b = b0 + k
            assert (x, y, score) == (int(got["anchor_x"][b]), int(got["anchor_y"][b]), int(got["anchor_score"][b])), (r, k)
            assert path == got["anchor_path"][int(got["anchor_path_off"][b]):int(got["anchor_path_off"][b + 1])].tolist(), (r, k)
            assert first == (int(got["anchor_first_node"][b]), int(got["anchor_first_offset"][b]), int(got["anchor_first_seqpos"][b])), (r, k)
            assert last == (int(got["anchor_last_node"][b]), int(got["anchor_last_offset"][b]), int(got["anchor_last_seqpos"][b])), (r, k)
        alignments += a1 - a0
        anchors += b1 - b0
    assert alignments >= 4 and anchors >= 20, (alignments, anchors)


def test_hits_a_kernel_would_read_out_of_bounds_through_are_refused(gca, golden_dir):
    """node_offset equal to the node's size, seq_pos equal to the read's length, a node the graph does not have: GC_ERR_INVALID from gc_seeds_upload with the hit's read and index,
    found by the resolve kernel's bounds checks before anything is loaded through the hit. The host's checks (offsets, read count) answer before that."""
    gfa = os.path.join(golden_dir, "syn20k.gfa")
    reads = [l.strip().encode() for l in open(os.path.join(golden_dir, "syn20k.fa")) if not l.startswith(">")][:3]
    graph = gca.AlignmentGraph(gfa)
    batch = gca.ReadBatch(reads)
    node_ids, node_offset, node_length = graph.array("nodeIDs"), graph.array("nodeOffset"), graph.array("nodeLength")
    big = int(node_ids[0])
    size = int(max(o + l for i, o, l in zip(node_ids, node_offset, node_length) if i == big))
    assert len(reads[1]) <= min(len(r) for r in reads)
    good = (big // 2, size - 1, len(reads[1]) - 1, 15, 0, big & 1)   # (the node's last base, the read's last base: inside)
    gca.SeedBatch(graph, batch, [[good], [good, good], []]).close()
    for bad, said in (((big // 2, size, 0, 15, 0, big & 1), "node_offset"), ((big // 2, 0, len(reads[1]), 15, 0, big & 1), "seq_pos"), ((int(node_ids.max()) // 2 + 1, 0, 0, 15, 0, 0), "no such node")):
        with pytest.raises(RuntimeError) as err:
            gca.SeedBatch(graph, batch, [[good], [good, bad, bad], [bad]])
        assert "error -1" in str(err.value) and "read 1 hit 1" in str(err.value) and said in str(err.value), str(err.value)
    with pytest.raises(RuntimeError, match="raw_goodness"):
        gca.SeedBatch(graph, batch, [[good], [(big // 2, 0, 0, 15, 0xffffffff, big & 1)], []])
    lib = gca.load_library()
    hits = np.array([good, good], dtype=gca.api.SEED_HIT_DTYPE)
    handle = C.c_void_p()
    for offsets, n in (([0, 2, 1, 2], 3), ([1, 1, 2, 2], 3), ([0, 1, 2], 2)):
        off = np.array(offsets, dtype=np.uint64)
        assert lib.gc_seeds_upload(graph.handle, batch.handle, hits.ctypes.data, off.ctypes.data, n, C.byref(handle)) == -1 and not handle.value
    # seeds made for one batch do not go with another
    seeds = gca.SeedBatch(graph, batch, [[good], [], []])
    other = gca.ReadBatch(reads[:2] + [reads[2][:-1]])
    with pytest.raises(RuntimeError, match="another read batch"):
        gca.Aligner(graph, None).align_batch(other, seeds=seeds)
