"""tests/bam_model.py against itself and against tests/golden/bam: its reader on the committed files, whose expected reads were written down by hand; the hand-spelled record;
and writer -> reader on random records. The model is the specification restated twice (its docstring says why), so this is what holds the two restatements together."""
import importlib.util
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bam_model as bm                             # noqa: E402
import bgzf_model                                  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "bam")


def _generator():
    spec = importlib.util.spec_from_file_location("make_bam_golden", os.path.join(GOLDEN, "make_bam_golden.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_the_reader_on_the_committed_files():
    expected = json.load(open(os.path.join(GOLDEN, "expected.json")))
    assert sorted(expected) == sorted(n for n in os.listdir(GOLDEN) if n.endswith(".bam")) and len(expected) >= 3
    for name, want in expected.items():
        data = open(os.path.join(GOLDEN, name), "rb").read()
        assert data.endswith(bgzf_model.EOF)
        ids, reads, skipped = bm.read_file(data)
        assert ([i.decode() for i in ids], reads, skipped) == (want["ids"], want["reads"], want["skipped"]), name
    assert set("".join(r for want in expected.values() for r in want["reads"])) == set(bm.LETTERS)
    assert any(want["skipped"] for want in expected.values()) and any("" in want["reads"] for want in expected.values())


def test_the_committed_files_are_what_the_generator_writes():
    """By their inflated bytes: zlib versions may deflate differently. The hand-spelled record is the writer's record too."""
    gen = _generator()
    for name, data in gen.build().items():
        assert bm.inflate(data) == bm.inflate(open(os.path.join(GOLDEN, name), "rb").read()), name
    assert gen.FILES == json.load(open(os.path.join(GOLDEN, "expected.json")))
    assert gen.HAND_RECORD == bm.record(b"r1", "=GNTGCAA", 0x14, (8 << 4 | 4,), b"NMC\x00", bytes([30]) * 8)
    assert gen.HAND_HEADER == bm.header(b"", ())
    assert bm.inflate(open(os.path.join(GOLDEN, "hand.bam"), "rb").read()) == gen.HAND_HEADER + gen.HAND_RECORD


def test_writer_to_reader_round_trip_on_random_records():
    rng = random.Random(4)
    for k in range(30):
        records = bm.random_records(rng, rng.randrange(0, 25), letters=bm.LETTERS)
        refs = ((b"chr1", 1000), (b"chr2", 5))[:k % 3]
        ids, reads, skipped = bm.read_file(bm.write(records, block_sizes=(rng.choice((1, 5, 37, 200, 65280)),), refs=refs))
        kept = [r for r in records if not r[2] & 0x900]
        assert skipped == len(records) - len(kept) and ids == [r[0] for r in kept]
        assert reads == [bm.revcomp(r[1]) if r[2] & 0x10 else r[1] for r in kept]
    assert bm.revcomp("ACGTMRWSYKVHDBN=") == "=NVHDBMRSWYKACGT"
    for a, b in bm.COMPLEMENT.items():                       # the complement by meaning is the 4-bit reversal of the code
        code = bm.LETTERS.index(a)
        assert bm.LETTERS.index(b) == int(f"{code:04b}"[::-1], 2)


def test_the_reader_names_what_it_refuses():
    good = [bm.record(b"a", "ACGT"), bm.record(b"b", "AC", 0x100), bm.record(b"c", "ACGTT", 0x10)]
    head = bm.header()
    for what, why in (("block_size", "block_size"), ("name", "name"), ("name0", "name"), ("l_seq", "l_seq"), ("span", "span")):
        data = head + good[0] + good[1] + bm.damaged(good[2], what)
        try:
            bm.read_stream(data)
            raise AssertionError(what)
        except bm.BamRefused as e:
            assert (e.record, e.offset, e.why) == (2, len(head) + len(good[0]) + len(good[1]), why)
    whole = head + b"".join(good)
    for cut in range(len(whole)):
        ids, reads, skipped, consumed = bm.read_stream(whole[:cut], final=False)
        assert consumed in (0, len(head), len(head) + len(good[0]), len(head) + len(good[0]) + len(good[1])) and consumed <= cut
        try:
            bm.read_stream(whole[:cut], final=True)
            assert cut == consumed >= len(head)                  # a cut behind the header or a record: a whole file
        except bm.BamRefused as e:
            assert e.why == "cut"
