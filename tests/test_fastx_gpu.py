"""The device FASTA / FASTQ loader (gc_reads_parse, ReadBatch.from_text) against tests/fastx_model.py, and the read batch it builds against the one ReadBatch(list) builds."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fastx_model as fm                           # noqa: E402
from test_fastx_model import fixture_cases         # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gca():
    import graphchainer_amd as g
    assert g.device_count() >= 1, "GPU tests need a device"
    return g


def check(gca, text, fmt, final):
    want_ids, want_seqs, want_consumed = fm.parse(text, fmt, final)
    batch, ids, consumed = gca.ReadBatch.from_text(text, fmt, final=final)
    try:
        where = (fmt, final, text[:200])
        assert consumed == want_consumed, where
        assert ids == want_ids, where
        assert [int(x) for x in batch.lengths] == [len(s) for s in want_seqs], where
        assert int(batch.offsets[0]) == 0 and np.array_equal(np.diff(batch.offsets), batch.lengths)
        assert batch.blob == b"".join(want_seqs), where
    finally:
        batch.close()


def test_fixtures_equal_the_model(gca):
    for name, fmt, text in fixture_cases():
        for other in ("fasta", "fastq"):          # (a file read as the other format is a text like any other)
            for final in (True, False):
                check(gca, text, other, final)


def test_random_texts_equal_the_model(gca):
    """The host program's seeded texts: every length around the kernels' tile sizes, and every fifth of the small ones; the format and the final flag by turns."""
    texts = fm.random_texts()
    around_tiles = 9 * len(fm.TILE_SIZES)          # (the list ends with them)
    big, small = texts[-around_tiles:], texts[:-around_tiles][::5]
    assert {len(t) for t in big} == {k * t + d for t in fm.TILE_SIZES for k in (1, 2, 3) for d in (-1, 0, 1)} and len(small) >= 100
    calls = 0
    for k, text in enumerate(big + small):
        for fmt, final in ((("fasta", True), ("fastq", False)) if k & 1 else (("fastq", True), ("fasta", False))):
            check(gca, text, fmt, final)
            calls += 1
    assert 200 <= calls <= 600


def test_one_long_line_and_many_short_lines(gca):
    """The two ends of the gather: a 64 KiB read on one line (spread over sixteen blocks' spans), and 70 000 FASTA lines of one letter (a span crosses sixteen lines)."""
    rng = np.random.default_rng(5)
    long_read = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 65536))
    for text, fmt in ((b">long one\n" + long_read + b"\n", "fasta"), (b"@long one\n" + long_read + b"\n+\n" + b"I" * 65536 + b"\n", "fastq"), (b"@cut\n" + long_read, "fastq")):
        check(gca, text, fmt, True)
        check(gca, text + (b">next\n" if fmt == "fasta" else b"@next\n"), fmt, False)
    letters = bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 70000))
    text = b">first\n" + b"".join(letters[i:i + 1] + b"\n" for i in range(35000)) + b">second x\n\n" + b"".join(letters[i:i + 1] + b"\r\n" for i in range(35000, 70000))
    check(gca, text, "fasta", True)
    check(gca, text, "fasta", False)
    check(gca, b"\n" * 70000, "fasta", True)
    check(gca, b"", "fastq", True)
    check(gca, b"", "fasta", False)


def golden_reads(golden_dir):
    return [l.strip().encode() for l in open(os.path.join(golden_dir, "syn20k.fa")) if not l.startswith(">")]


def as_text(reads, style):
    if style == "fasta60":
        return b"".join(b">r%d\n" % i + b"".join(r[k:k + 60] + b"\n" for k in range(0, len(r), 60)) for i, r in enumerate(reads)), "fasta"
    eol = b"\r\n" if style == "fastq_crlf" else b"\n"
    return b"".join(b"@r%d" % i + eol + r + eol + b"+" + eol + b"I" * len(r) + eol for i, r in enumerate(reads)), "fastq"


@pytest.fixture(scope="module")
def golden_graph(gca, golden_dir):
    graph = gca.AlignmentGraph(os.path.join(golden_dir, "syn20k.gfa"))
    return graph, gca.MinimizerSeeder(graph)


def same_results(a, b):
    assert set(a) == set(b)
    for key in a:
        if key in ("kernel_us", "host_us", "counters", "counters_long"):   # timings and work statistics, not results
            continue
        if isinstance(a[key], (bytes, int)):
            assert a[key] == b[key], key
        else:
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key


@pytest.mark.parametrize("style", ["fasta60", "fastq", "fastq_crlf"])
def test_parsed_batch_aligns_as_the_uploaded_one(gca, golden_dir, golden_graph, style):
    """The six golden reads as FASTA of width 60, FASTQ and CRLF FASTQ: the batch parsed on the device gives every array ReadBatch(list) gives, through chaining with the
    whole-read pass and the writers."""
    graph, seeder = golden_graph
    reads = golden_reads(golden_dir)
    text, fmt = as_text(reads, style)
    parsed, ids, consumed = gca.ReadBatch.from_text(text, fmt)
    assert ids == [b"r%d" % i for i in range(len(reads))] and consumed == len(text)
    uploaded = gca.ReadBatch(reads)
    assert parsed.blob == uploaded.blob and np.array_equal(parsed.offsets, uploaded.offsets) and np.array_equal(parsed.lengths, uploaded.lengths)
    aligner = gca.Aligner(graph, seeder, long_pass=True, keep_traces=True, keep_seeds=True, chain_traces=2)
    got = aligner.align_batch(parsed, gaf_names=ids, other_formats=True)
    want = aligner.align_batch(uploaded, gaf_names=ids, other_formats=True)
    assert int(want["read_chain_off"][-1]) > 0 and want["gaf"]
    same_results(got, want)
    assert got["gaf"] == open(os.path.join(golden_dir, "syn20k.expected.gaf"), "rb").read()


def test_parsed_batch_seeds_as_the_uploaded_one_with_an_mxm_index(gca, golden_dir, golden_graph):
    graph, _ = golden_graph
    reads = golden_reads(golden_dir)
    text, fmt = as_text(reads, "fasta60")
    parsed, ids, _ = gca.ReadBatch.from_text(text, fmt)
    uploaded = gca.ReadBatch(reads)
    index = gca.MxmIndex(graph)
    s_parsed, s_uploaded = index.seeds(parsed, "mem", count=100, min_len=20), index.seeds(uploaded, "mem", count=100, min_len=20)
    hits = s_uploaded.hits()
    assert sum(len(h) for h in hits) > 0
    for a, b in zip(s_parsed.hits(), hits):
        assert np.array_equal(a, b)
    aligner = gca.Aligner(graph, None, long_pass=True, keep_traces=2)
    same_results(aligner.align_batch(parsed, seeds=s_parsed, gaf_names=ids), aligner.align_batch(uploaded, seeds=s_uploaded, gaf_names=ids))


def test_chunks(gca, golden_dir, tmp_path):
    """A text fed in chunks of 3 000 bytes gives the same reads in the same order, from a plain file and from a gzipped one of two members; files are not joined."""
    import gzip
    reads = golden_reads(golden_dir)
    for style, suffix in (("fasta60", ".fa"), ("fastq", ".fq")):
        text, fmt = as_text(reads, style)
        plain, packed, last = tmp_path / ("reads" + suffix), tmp_path / ("reads" + suffix + ".gz"), tmp_path / ("tail" + suffix)
        plain.write_bytes(text)
        cut = text.index(b"r3") - 1
        packed.write_bytes(gzip.compress(text[:cut]) + gzip.compress(text[cut:]))
        last.write_bytes(text[:cut][:-1])          # ends without a newline: the end-of-file rules apply to it, not to the file in front of it
        (tmp_path / "ignored.txt").write_bytes(text)
        want_tail = fm.parse(text[:cut][:-1], fmt)
        for path in (plain, packed):
            got_ids, got_reads, batches = [], [], 0
            for batch, ids in gca.read_files([str(path), str(tmp_path / "ignored.txt"), str(last)], batch_bytes=3000):
                got_ids += ids
                got_reads += [batch.blob[int(batch.offsets[i]):int(batch.offsets[i + 1])] for i in range(len(ids))]
                batches += 1
                batch.close()
            assert got_ids == [b"r%d" % i for i in range(len(reads))] + want_tail[0]
            assert got_reads == reads + want_tail[1]
            assert batches >= 4
