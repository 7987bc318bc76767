"""Seeds from GAM files on the GPU (gc_seed_store_open / gc_seeds_from_store; SeedStore; the command's -s), held to tests/seedfile_model.py - the reference's reader and
its map from read name to hits - with seed records from the seeding model, as tests/test_seed_hits_gpu.py takes them:
  1. SeedStore.seeds(...).hits() is the model's list, read by read: 63, 64, 65 and 257 seeds of one read, a message larger than the decode kernel's LDS tile, pieces of a few
     hundred bytes (one message longer than a piece), a multi-member gzip file and a zlib one;
  2. the join: absent reads, names that are prefixes of one another, the empty name, one name twice in a batch, one name in two files and in both file orders, a batch without
     any seed - with the whole hash and with 2 bits of it, where every lookup walks foreign names;
  3. align_batch on the store's seeds returns what it returns on SeedBatch(model hits), key for key; values gc_seed_hit cannot hold are refused by read and hit;
  4. the command with -s writes the API path's bytes; a missing file ends it with status 0, a damaged one with status 1, both without output."""
import gzip
import os
import random
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import seedfile_model as sm                                 # noqa: E402
import seeding_model                                        # noqa: E402
from graphchainer_amd.synth import SynthGraph              # noqa: E402  (test inputs)
from test_cli_gpu import fasta, gam_messages                # noqa: E402
from test_gpu_parity import gca                             # noqa: E402,F401  (the fixture)
from test_seeding_model import _inputs, std_sort            # noqa: E402,F401  (the fixture)

pytestmark = pytest.mark.gpu

TIMING_KEYS = ("kernel_us", "host_us", "counters", "counters_long")   # times, and counts of reruns that depend on what the process ran before


def _model_hits(gfa, reads, std_sort):   # noqa: F811
    """Per read the minimizer model's hits as a seeds file can carry them: (node_id, node_offset, seq_pos, match_len, reverse)."""
    from oracle import Oracle
    oracle = Oracle(gfa, long_pass=False)                   # (its graph and index arrays are the model's inputs; it aligns nothing here)
    graph, index = _inputs(oracle)
    return [[(s["nodeID"], s["nodeOffset"], s["seqPos"], s["matchLen"], int(s["reverse"])) for s in seeding_model.get_seeds(read, index, graph, 15, 20, 10.0, std_sort)] for read in reads]


def _messages(name, hits):
    return [sm.seed_message(name, node, off, pos, length, rev) for node, off, pos, length, rev in hits]


@pytest.fixture(scope="module")
def synth(gca, tmp_path_factory, std_sort):   # noqa: F811
    """One small graph, four reads and their model hits, computed once and left unchanged."""
    tmp = tmp_path_factory.mktemp("seedfile")
    sg = SynthGraph(40_000, seed=37)
    gfa = str(tmp / "g.gfa")
    sg.write_gfa(gfa)
    reads = sg.sample_reads(4, 1500, seed=6, p_del=0.01, p_sub=0.01, p_ins=0.01)
    hits = _model_hits(gfa, reads, std_sort)
    assert min(len(h) for h in hits) >= 40
    return {"gfa": gfa, "graph": gca.AlignmentGraph(gfa), "reads": reads, "hits": hits}


def _expected(files, ids):
    """The model: every file inflated and read in order, then the lookup by name."""
    seeds = sm.seed_map([sm.inflate(data) for data in files])
    return [seeds.get(i, []) for i in ids]


def _as_lists(per_read):
    return [[tuple(int(x) for x in h) for h in hits.tolist()] for hits in per_read]


def test_hits_equal_the_model_read_by_read(gca, synth, tmp_path, monkeypatch):
    monkeypatch.setenv("GC_TEST_SEEDFILE_PIECE", "700")
    base, reads = synth["hits"], synth["reads"]
    long_name = b"a read with a very long header line " * 9
    counts = {b"c63": 63, b"c64": 64, b"c65": 65, b"c257": 257}
    ids = [b"c63", b"c64", b"c65", b"c257", b"plain", long_name, b"big"]
    batch_reads = [reads[0]] * 4 + [reads[1], reads[2], reads[3]]
    groups = []
    for name, n in counts.items():
        groups.append(_messages(name.decode(), [base[0][k % len(base[0])] for k in range(n)]))
    groups.append(_messages("plain", base[1]))
    groups.append([])
    groups.append(_messages(long_name.decode(), base[2]) + [b""])
    big = _messages("big", base[3][:3])
    big[1] += sm.varint(11 << 3 | 2) + sm.varint(9000) + bytes(k % 251 for k in range(9000))    # an unknown field: the message is larger than the LDS tile and than a piece
    groups.append(big)
    raw = sm.write_stream(groups)
    raw2 = sm.write_stream([groups[6], groups[4]])          # the second file: two of the names again, in the other order
    first, second = tmp_path / "first.gam", tmp_path / "second.gam"
    sm.write_file(first, [raw[:1000], raw[1000:1001], raw[1001:]], "gzip")     # three gzip members, cut inside messages
    sm.write_file(second, [raw2], "zlib")
    store = gca.SeedStore([str(first), str(second)])
    want = _expected([first.read_bytes(), second.read_bytes()], ids)
    assert [len(w) for w in want] == [63, 64, 65, 257, 2 * len(base[1]), 2 * len(base[2]), 3]
    batch = gca.ReadBatch(batch_reads)
    seeds = store.seeds(synth["graph"], batch, ids)
    assert _as_lists(seeds.hits()) == want
    info = store.info()
    total = sum(len(g) for g in sm.seed_map([raw, raw2]).values())
    assert info["seeds"] == total and info["messages"] == total + 2 and info["distinct_hashes"] == len(ids)
    assert info["hbm_bytes"] >= 48 * total and info["device_ms"] > 0 and seeds.kernel_ms > 0
    # the same store from inflated streams, in one piece
    monkeypatch.delenv("GC_TEST_SEEDFILE_PIECE")
    again = gca.SeedStore(streams=[raw, raw2])
    assert _as_lists(again.seeds(synth["graph"], batch, ids).hits()) == want


@pytest.mark.parametrize("hash_bits", [64, 2])
def test_the_join(gca, synth, hash_bits, monkeypatch):
    if hash_bits != 64:
        monkeypatch.setenv("GC_TEST_SEEDFILE_HASH_BITS", str(hash_bits))
    base, reads, graph = synth["hits"], synth["reads"], synth["graph"]
    half = len(base[0]) // 2
    file_a = sm.write_stream([_messages("r1", base[0][:half]), _messages("r10", base[1]), _messages("", base[2][:10])])
    file_b = sm.write_stream([_messages("", base[2][10:20]) + _messages("r1", base[0][half:]), _messages("r100", base[3])])
    ids = [b"r1", b"r10", b"", b"r1", b"absent", b"r", b"r100"]
    batch = gca.ReadBatch([reads[0], reads[1], reads[2], reads[0], reads[3], reads[3], reads[3]])
    for streams in ([file_a, file_b], [file_b, file_a]):
        store = gca.SeedStore(streams=streams)
        want = [sm.seed_map(streams).get(i, []) for i in ids]
        got = _as_lists(store.seeds(graph, batch, ids).hits())
        assert got == want and got[0] == got[3] and got[4] == got[5] == [] and len(got[2]) == 20
        assert store.info()["distinct_hashes"] == 4 if hash_bits == 64 else 1 <= store.info()["distinct_hashes"] <= 4    # r1, r10, r100 and the empty name
        none = store.seeds(graph, batch, [b"x%d" % k for k in range(7)])     # a batch in which no read has a seed
        assert _as_lists(none.hits()) == [[]] * 7
        assert np.asarray(gca.Aligner(graph, None).align_batch(batch, seeds=none)["read_seed_off"]).tolist() == [0] * 8
    in_order = _as_lists(gca.SeedStore(streams=[file_a, file_b]).seeds(graph, batch, ids).hits())[0]
    swapped = _as_lists(gca.SeedStore(streams=[file_b, file_a]).seeds(graph, batch, ids).hits())[0]
    assert in_order == swapped[len(base[0]) - half:] + swapped[:len(base[0]) - half] and in_order != swapped   # the first file's hits first
    empty = gca.SeedStore(streams=[b"", sm.write_stream([0])])
    assert empty.info()["seeds"] == 0 and _as_lists(empty.seeds(graph, batch, ids).hits()) == [[]] * 7


def _same(got, want):
    assert got.keys() == want.keys()
    for key in got:
        if key in TIMING_KEYS:
            continue
        if isinstance(got[key], (bytes, int)):
            assert got[key] == want[key], key
        else:
            assert np.array_equal(np.asarray(got[key]), np.asarray(want[key])), key


def _both_ways(gca, graph, reads, ids, streams):
    batch = gca.ReadBatch(reads)
    want_hits = [sm.seed_map(streams).get(i, []) for i in ids]
    kw = dict(keep_traces=True, keep_seeds=True, long_pass=True, chain_traces=2)
    want = gca.Aligner(graph, None, **kw).align_batch(batch, seeds=gca.SeedBatch(graph, batch, want_hits), gaf_names=ids, formats=("gaf", "gam"))
    got = gca.Aligner(graph, None, **kw).align_batch(batch, seeds=gca.SeedStore(streams=streams).seeds(graph, batch, ids), gaf_names=ids, formats=("gaf", "gam"))
    _same(got, want)
    return want


def test_alignments_on_the_stores_seeds_equal_those_on_uploaded_hits(gca, synth, golden_dir, std_sort):   # noqa: F811
    base, reads, graph = synth["hits"], synth["reads"], synth["graph"]
    ids = [b"read %d" % k for k in range(4)]
    # the minimizer hits as the file's content
    want = _both_ways(gca, graph, reads, ids, [sm.write_stream([_messages(i.decode(), h) for i, h in zip(ids, base)])])
    assert int(want["read_seed_off"][-1]) == sum(len(h) for h in base) and want["gaf"].count(b"\n") >= 3
    # the reference's own test graph and read
    gfa = os.path.join(golden_dir, "ref_test_graph.gfa")
    ref_read = [open(os.path.join(golden_dir, "ref_test_read.fa")).read().split("\n")[1].encode()]
    ref_hits = _model_hits(gfa, ref_read, std_sort)
    assert ref_hits[0]
    _both_ways(gca, gca.AlignmentGraph(gfa), ref_read, [b"read"], [sm.write_stream([_messages("read", ref_hits[0])])])
    # hits the minimizer path cannot produce: thinned, shuffled, other lengths, a duplicate, a read without any
    rng = random.Random(5)
    foreign = []
    for h in base:
        kept = [(n, o, p, rng.randint(2, 60), r) for n, o, p, _, r in h[::3]]
        rng.shuffle(kept)
        foreign.append(kept + kept[:1])
    foreign[2] = []
    want = _both_ways(gca, graph, reads, ids, [sm.write_stream([_messages(i.decode(), h) for i, h in zip(ids, foreign)])])
    assert int(want["read_seed_off"][1]) > 0 and int(want["read_seed_off"][3]) == int(want["read_seed_off"][2])


def test_values_a_seed_hit_cannot_hold_are_refused_by_read_and_hit(gca, synth):
    base, reads, graph = synth["hits"], synth["reads"], synth["graph"]
    ids = [b"a", b"b", b"c"]
    batch = gca.ReadBatch(reads[:3])
    good = base[1][0]
    for bad, said in (((good[0], -1, good[2], 15, good[4]), "node_offset"), ((good[0], 1 << 33, good[2], 15, good[4]), "node_offset"), ((good[0], good[1], -1, 15, good[4]), "seq_pos"),
                      ((good[0], good[1], len(reads[1]), 15, good[4]), "seq_pos"), ((1 << 30, 0, 0, 15, 0), "no such node"), ((good[0], good[1], good[2], -3, good[4]), "match_len")):
        stream = sm.write_stream([_messages("a", base[0][:2]), _messages("b", [good, bad, bad]), _messages("c", [bad])])
        store = gca.SeedStore(streams=[stream])               # the store takes the values as they are ...
        with pytest.raises(RuntimeError) as err:
            store.seeds(graph, batch, ids)                    # ... and the join refuses them, as gc_seeds_upload refuses them
        assert "error -1" in str(err.value) and "read 1 hit 1" in str(err.value) and said in str(err.value), str(err.value)
    for stream, said in ((sm.write_stream([[sm.seed_message("a", 1, 2, 3, 4, False), b"\x1a\x05ab"]]), "file 0 message 1 does not parse"),
                         (sm.write_stream([[b"\x1a\x01a"]]), "file 0 message 0 has no mapping"), (sm.write_stream([[b"\x12\x04\x12\x02\x0a\x00"]]), "without an edit"),
                         (sm.write_stream([[sm.seed_message("a", 1, 2, 3, 4, False)]])[:-1], "runs past the end"), (sm.write_stream([3]), "runs past the end")):
        with pytest.raises(RuntimeError) as err:
            gca.SeedStore(streams=[b"", stream] if "file 0" not in said else [stream])
        assert "error -1" in str(err.value) and said in str(err.value) and ("file 0" in said or "file 1" in str(err.value)), str(err.value)


def _command(*args):
    return subprocess.run([sys.executable, "-m", "graphchainer_amd"] + [str(a) for a in args], capture_output=True, text=True, timeout=300, cwd=ROOT)


def test_the_command_with_a_seeds_file(gca, synth, tmp_path):
    base, reads, graph = synth["hits"], synth["reads"], synth["graph"]
    ids = [b"r%d some description" % k for k in range(4)]
    (tmp_path / "reads.fa").write_bytes(fasta(reads, ids))
    raw = sm.write_stream([_messages(i.decode(), h) for i, h in zip(ids[:3], base)])       # (the last read has no entry)
    sm.write_file(tmp_path / "seeds.gam", [raw[:777], raw[777:]])
    out = _command("-g", synth["gfa"], "-f", tmp_path / "reads.fa", "-s", tmp_path / "seeds.gam", "--seeds-minimizer-density", "0", "-a", tmp_path / "out.gaf", "-a", tmp_path / "out.gam")
    assert out.returncode == 0, out.stdout + out.stderr
    batch = gca.ReadBatch(reads)
    hits = [sm.seed_map([raw]).get(i, []) for i in ids]
    want = gca.Aligner(graph, None, long_pass=True, keep_traces=2, seed_density=0.0).align_batch(batch, seeds=gca.SeedBatch(graph, batch, hits), gaf_names=ids, formats=("gaf", "gam"))
    assert want["gaf"].count(b"\n") >= 3
    assert (tmp_path / "out.gaf").read_bytes() == want["gaf"]
    assert gam_messages((tmp_path / "out.gam").read_bytes()) == gam_messages(want["gam"])
    # a file that is not there: said, status 0, nothing written
    out = _command("-g", synth["gfa"], "-f", tmp_path / "reads.fa", "-s", tmp_path / "seeds.gam", tmp_path / "missing.gam", "--seeds-minimizer-density", "0", "-a", tmp_path / "none.gaf")
    assert out.returncode == 0 and out.stderr == "No seeds file exists\n" and not (tmp_path / "none.gaf").exists()
    # a damaged file: status 1, nothing written
    (tmp_path / "cut.gam").write_bytes(gzip.compress(raw[:-3]))
    (tmp_path / "text.gam").write_bytes(raw)
    for name in ("cut.gam", "text.gam"):
        out = _command("-g", synth["gfa"], "-f", tmp_path / "reads.fa", "-s", tmp_path / name, "--seeds-minimizer-density", "0", "-a", tmp_path / "bad.gaf")
        assert out.returncode == 1 and "seeds file" in out.stderr and len(out.stderr.splitlines()) == 1, out.stderr
    assert sorted(p.name for p in tmp_path.iterdir()) == ["cut.gam", "out.gaf", "out.gam", "reads.fa", "seeds.gam", "text.gam"]
