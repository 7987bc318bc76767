"""tests/fastx_model.py, the model the device loader (gc_reads_parse) is held to, against what the reference's own reader
yielded on the fixtures of tests/golden/fastx (recorded by tests/golden/make_fastx_golden.py), and the chunk protocol in
the model itself."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fastx_model as fm                       # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
EXPECTED = json.load(open(os.path.join(GOLDEN, "fastx.expected.json")))


def fixture_text(name):
    return open(os.path.join(GOLDEN, "fastx", name), "rb").read()


def fixture_cases():
    """(name, format, text) of every fixture whose name selects a format."""
    return [(name, fm.file_format(name)[0], fixture_text(name)) for name in sorted(EXPECTED) if fm.file_format(name)[0]]


def test_the_fixtures_are_the_recorded_ones():
    assert len(EXPECTED) >= 20 and sorted(EXPECTED) == sorted(os.listdir(os.path.join(GOLDEN, "fastx")))
    # the eight cases of the specification, as the reference answered them
    pairs = lambda name: list(zip(EXPECTED[name]["ids"], EXPECTED[name]["sequences"]))   # noqa: E731
    assert pairs("case1.fa") == [("a x y", "ACGTAC"), ("b", "")]
    assert pairs("case2_crlf.fa") == [("a", "ACGT"), ("b", ""), ("c", "T")]
    assert pairs("case3_junk.fa") == [("a", "AC")]
    assert pairs("case4.fq") == [("a d", "ACGT"), ("b", "GG")]
    assert pairs("case5.fq") == [("a", "AC"), ("b", "GG")]
    assert pairs("case6_empty.fa") == [] and pairs("case6_empty.fq") == []
    assert pairs("case7_header_only.fa") == [("a", "")] and pairs("case8_header_line.fa") == [("a", "")]


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_model_reproduces_the_reference_on_every_fixture(name):
    fmt, gz = fm.file_format(name)
    want = EXPECTED[name]
    if fmt is None:      # another file name: no reads and no error
        assert want == {"ids": [], "sequences": []}
        return
    text = fixture_text(name)
    ids, seqs, consumed = fm.parse(text, fmt)
    assert [i.decode("latin-1") for i in ids] == want["ids"]
    assert [s.decode("latin-1") for s in seqs] == want["sequences"]
    assert consumed == len(text) and not gz


def test_file_names_select_the_format_as_the_reference_does():
    assert fm.file_format("x.fa") == ("fasta", False) and fm.file_format("x.fasta.gz") == ("fasta", True)
    assert fm.file_format("x.fq") == ("fastq", False) and fm.file_format("x.fastq.gz") == ("fastq", True)
    assert fm.file_format("reads.txt") == (None, False) and fm.file_format("x.fa.bz2") == (None, False) and fm.file_format("x.FA") == (None, False)
    assert fm.file_format(".fa") == (None, False) and fm.file_format(".gz") == (None, False) and fm.file_format("a.fa") == ("fasta", False)   # size() > 3, as the reference tests it


def test_model_reads_the_golden_reads_as_the_tests_do(golden_dir):
    path = os.path.join(golden_dir, "syn20k.fa")
    want = [l.strip() for l in open(path) if not l.startswith(">")]
    ids, seqs, _ = fm.parse(open(path, "rb").read(), "fasta")
    assert [s.decode() for s in seqs] == want and len(ids) == len(want) == 6


@pytest.mark.parametrize("name,fmt,text", fixture_cases(), ids=[c[0] for c in fixture_cases()])
def test_chunks_cut_at_every_byte_give_the_whole_file(name, fmt, text):
    """A chunk without final yields only records whose end it has seen; what it leaves is carried over. Cutting at any byte, or at any two, changes nothing."""
    whole = fm.parse(text, fmt)[:2]
    for cut in range(len(text) + 1):
        assert fm.parse_chunks(text, fmt, [cut]) == whole, cut
    step = max(1, len(text) // 25)
    for a in range(0, len(text) + 1, step):
        for b in range(a, len(text) + 1, step):
            assert fm.parse_chunks(text, fmt, [a, b]) == whole, (a, b)


def test_a_chunk_without_a_complete_record_consumes_nothing():
    assert fm.parse(b">a\nACGT\n", "fasta", final=False) == ([], [], 0)          # the next header has not been seen
    assert fm.parse(b">a\nACGT\n>b", "fasta", final=False) == ([], [], 0)        # ... not as a whole line
    assert fm.parse(b">a\nACGT\n>b\n", "fasta", final=False) == ([b"a"], [b"ACGT"], 8)
    assert fm.parse(b"@a\nAC\n+\nII", "fastq", final=False) == ([], [], 0)
    assert fm.parse(b"@a\nAC\n+\nII\n@b\nGG\n", "fastq", final=False) == ([b"a"], [b"AC"], 11)
    assert fm.parse(b"", "fastq", final=False) == ([], [], 0) and fm.parse(b"", "fasta", final=False) == ([], [], 0)
