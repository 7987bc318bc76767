"""Unaligned BAM decoded on the device (ReadBatch.from_bam, from_bam_bgzf) against tests/bam_model.py: the reads, ids and skipped count of the model's reader for the bytes of
the model's writer, the batch ReadBatch(list of the reads) builds, the chunk protocol at every kind of cut, the BGZF path at block sizes that put a boundary inside every
field, every refusal, and a read that holds '='."""
import os
import random
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bam_model as bm                             # noqa: E402

pytestmark = pytest.mark.gpu

ALL = "=ACMGRSVTWYHKDBN"


@pytest.fixture(scope="module")
def gca():
    import graphchainer_amd as g
    assert g.device_count() >= 1, "GPU tests need a device"
    return g


def golden_reads(golden_dir):
    return [l.strip() for l in open(os.path.join(golden_dir, "syn20k.fa")) if not l.startswith(">")]


@pytest.fixture(scope="module")
def big(golden_dir):
    """The records of test 1: every length at which the unpacking takes another path, a record longer than the walk's window between small ones, both name lengths, every
    code, every flag, CIGAR ops and tags - and the six golden reads, three of them stored on the reverse strand, so that the alignment below has something to align."""
    rng = random.Random(11)
    letters = lambda n, alphabet="ACGT": "".join(rng.choice(alphabet) for _ in range(n))   # noqa: E731
    records = []
    for k, length in enumerate((0, 1, 2, 15, 16, 17, 31, 32, 33, 4097)):
        for flag in (0, 4, 0x10, 0x14):
            records.append((b"len%d/%x" % (length, flag), letters(length, "ACGTN" if k % 2 else "ACGT"), flag, tuple(range(k % 4)), rng.randbytes(k * 3)))
    records.insert(7, (b"w", letters(40000), 0x10, (40000 << 4,), b"NMC\x00"))                # larger than the walk's window, between small ones
    records.insert(3, (b"n" * 254, letters(50), 0))
    records.insert(9, (b"1", ALL, 4))
    records.insert(12, (b"codes/rc", ALL + ALL[::-1] + "A", 0x14, (1, 2, 3), b"xyZabc\x00"))
    records.insert(5, (b"secondary", letters(33), 0x100, (33 << 4,)))
    records.insert(20, (b"supplementary", letters(17), 0x810))
    for k, read in enumerate(golden_reads(golden_dir)):
        records.append((b"golden%d" % k, bm.revcomp(read) if k % 2 else read, 0x10 if k % 2 else 0, (len(read) << 4,), b"RGZa\x00"))
    return records


@pytest.fixture(scope="module")
def graph(gca, golden_dir):
    g = gca.AlignmentGraph(os.path.join(golden_dir, "syn20k.gfa"))
    return g, gca.MinimizerSeeder(g)


def same_results(a, b):
    assert set(a) == set(b)
    for key in a:
        if key in ("kernel_us", "host_us", "counters", "counters_long"):   # timings and work statistics, not results
            continue
        if isinstance(a[key], (bytes, int)):
            assert a[key] == b[key], key
        else:
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key


@pytest.mark.parametrize("refs", [(), ((b"chr1", 1000), (b"chr2", 1 << 31), (b"x", 1))])
def test_one_stream_equals_the_model_and_the_uploaded_batch(gca, big, graph, refs):
    data = bm.stream(big, refs=refs)
    ids, reads, skipped, consumed = bm.read_stream(data)
    assert skipped == 2 and {len(r) for r in reads} >= {0, 1, 2, 15, 16, 17, 31, 32, 33, 4097, 40000} and {len(i) for i in ids} >= {1, 254} and set("".join(reads)) == set(ALL)
    batch, got_ids, got_consumed = gca.ReadBatch.from_bam(data, header=True)
    assert got_ids == ids and got_consumed == consumed == len(data)
    assert batch.bam["skipped"] == skipped and batch.bam["records"] == len(big)
    uploaded = gca.ReadBatch(reads)
    assert batch.blob == uploaded.blob == "".join(reads).encode()
    assert np.array_equal(batch.offsets, uploaded.offsets) and np.array_equal(batch.lengths, uploaded.lengths)
    aligner = gca.Aligner(*graph, long_pass=True, keep_traces=True, keep_seeds=True, chain_traces=2)
    got = aligner.align_batch(batch, gaf_names=ids, other_formats=True)
    want = aligner.align_batch(uploaded, gaf_names=ids, other_formats=True)
    assert int(want["read_chain_off"][-1]) > 0 and want["gaf"].count(b"\n") >= 6
    same_results(got, want)
    batch.close()
    uploaded.close()


@pytest.fixture(scope="module")
def small():
    """About 3 KB: a header with two references, then records of every kind."""
    rng = random.Random(3)
    records = [(b"first", "ACGTTGCAN", 0x10, (9 << 4,), b"ab"), (b"2", "", 0x100), (b"third", "G", 4)] + bm.random_records(rng, 32, max_len=120, letters=ALL)
    data = bm.stream(records, text=b"@HD\tVN:1.6\n", refs=((b"chr1", 10), (b"chr22", 20)))
    assert 2500 < len(data) < 4000
    return records, data


def test_chunk_protocol_at_every_kind_of_cut(gca, small):
    records, data = small
    ids, reads, skipped, _ = bm.read_stream(data)
    starts = [bm.read_header(data)]
    while starts[-1] < len(data):
        starts.append(bm.read_record(data, starts[-1], 0)[0])
    cuts = list(range(starts[2])) + list(range(starts[2], len(data) + 1, 7))
    assert 300 < len(cuts) < 700
    for cut in cuts:
        first, first_ids, consumed = gca.ReadBatch.from_bam(data[:cut], header=True, final=False)
        want = bm.read_stream(data[:cut], final=False)
        assert consumed == want[3] == max([0] + [s for s in starts if s <= cut]), cut
        assert (first_ids, first.blob.decode(), first.bam["skipped"]) == (want[0], "".join(want[1]), want[2]), cut
        rest, rest_ids, rest_consumed = gca.ReadBatch.from_bam(data[consumed:], header=consumed == 0, final=True)
        assert rest_consumed == len(data) - consumed, cut
        assert first_ids + rest_ids == ids and first.blob + rest.blob == "".join(reads).encode() and first.bam["skipped"] + rest.bam["skipped"] == skipped, cut
        assert [int(x) for x in first.lengths] + [int(x) for x in rest.lengths] == [len(r) for r in reads], cut
        first.close()
        rest.close()


@pytest.mark.parametrize("block", [1, 5, 37, 65280])
def test_the_bgzf_path_equals_the_plain_one(gca, small, big, block):
    """Blocks of 1, 5 and 37 bytes of text put a block boundary inside block_size, the fixed fields, a name and the bases; 65 280 is what bgzip writes. The piece is cut at
    a block boundary in its middle, so a non-empty head is carried from the first call to the second."""
    data = bm.stream(big) if block >= 37 else small[1]
    assert len(data) > block
    plain, ids, _ = gca.ReadBatch.from_bam(data, header=True)
    whole = bm.bgzf(data, (block,))
    batch, got_ids, tail, consumed = gca.ReadBatch.from_bam_bgzf(b"", whole, header=True)
    assert (got_ids, batch.blob, tail, consumed) == (ids, plain.blob, b"", len(whole)) and np.array_equal(batch.offsets, plain.offsets)
    assert batch.bam["skipped"] == plain.bam["skipped"] and batch.bgzf["inflated_bytes"] == len(data) and batch.bgzf["blocks"] == -(-len(data) // block) + 1   # the end-of-file block too
    import bgzf_model
    sizes, at = bgzf_model.bgzf_sizes(whole), 0
    for size in sizes[:max(1, (len(sizes) - 1) * 2 // 5)]:
        at += size
    a, a_ids, tail, consumed = gca.ReadBatch.from_bam_bgzf(b"", whole[:at], header=True, final=False)
    assert consumed == at and len(tail) > 0 and data[:a.bgzf["inflated_bytes"]].endswith(tail)
    b, b_ids, rest, consumed = gca.ReadBatch.from_bam_bgzf(tail, whole[at:], header=len(tail) == a.bgzf["inflated_bytes"], final=True)
    assert rest == b"" and consumed == len(whole) - at
    assert a_ids + b_ids == ids and a.blob + b.blob == plain.blob and a.bam["skipped"] + b.bam["skipped"] == plain.bam["skipped"]
    for x in (plain, batch, a, b):
        x.close()


def test_every_refusal_names_its_record_and_leaves_the_device_usable(gca):
    good = [bm.record(b"a", "ACGTACGTAC", 0, (1,)), bm.record(b"left out", "ACGT", 0x800), bm.record(b"c", "ACGTT", 0x10, (), b"tags")]
    victim = bm.record(b"victim", "ACGTACGTA", 4, (1, 2), b"tag")
    head = bm.header(refs=((b"chr1", 5),))
    at = len(head) + len(good[0]) + len(good[1])
    cases = [(head + good[0] + good[1] + bm.damaged(victim, what) + good[2], rf"record 2 at byte {at} ") for what in ("block_size", "name", "name0", "l_seq", "span")]
    cases.append((b"BAM\x02" + head[4:] + good[0], r"header at byte 0 "))
    cases.append((good[0] + good[1], r"header at byte 0 "))                                          # records where a header is expected
    cases.append((head[:-3], r"header at byte 0 "))                                                  # FINAL: the end cuts the header,
    cases.append((head + good[0] + good[1] + victim[:-1], rf"record 2 at byte {at} "))               # a record,
    cases.append((head + good[0] + good[1] + victim[:2], rf"record 2 at byte {at} "))                # a block_size word
    cases.append((head + bm.damaged(victim, "span") + bm.damaged(victim, "name0"), rf"record 0 at byte {len(head)} "))   # the first of two
    whole = head + b"".join(good)
    for data, names in cases:
        with pytest.raises(RuntimeError, match="graphchainer_amd error -1: gc_reads_parse_bam: .*" + names + "refused"):
            gca.ReadBatch.from_bam(data, header=True, final=True)
        batch, ids, consumed = gca.ReadBatch.from_bam(whole, header=True)                            # a good call on the same process
        assert ids == [b"a", b"c"] and batch.blob == b"ACGTACGTACAACGT" and batch.bam["skipped"] == 1 and consumed == len(whole)
        batch.close()
    data, names = cases[4]
    with pytest.raises(RuntimeError, match="gc_reads_parse_bam_bgzf: .*" + names + "refused"):
        gca.ReadBatch.from_bam_bgzf(b"", bm.bgzf(data, (50,)), header=True)
    batch, ids, tail, _ = gca.ReadBatch.from_bam_bgzf(b"", bm.bgzf(whole, (50,)), header=True)
    assert ids == [b"a", b"c"] and tail == b""
    batch.close()
    for flags_header, final in ((True, False), (False, False)):                                      # without FINAL a cut is no error
        batch, ids, consumed = gca.ReadBatch.from_bam(whole[:-1] if flags_header else whole[len(head):-1], header=flags_header, final=final)
        assert ids == [b"a"] and consumed == (len(whole) if flags_header else len(whole) - len(head)) - len(good[2])
        batch.close()
    lib = gca.load_library()                                                                         # the calls refused before a device is needed
    import ctypes as C
    lib.gc_reads_parse_bam.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    handle, table = C.c_void_p(), C.c_void_p()
    assert lib.gc_reads_parse_bam(whole, len(whole), 4, C.byref(handle), C.byref(table), None) == -1 and b"unknown flag bits" in lib.gc_last_error()
    assert lib.gc_reads_parse_bam(whole, 0xfffffff0, 3, C.byref(handle), C.byref(table), None) == -1 and b"2^32 - 16" in lib.gc_last_error()
    assert lib.gc_reads_parse_bam(whole, len(whole), 3, None, C.byref(table), None) == -1 and b"null argument" in lib.gc_last_error()


def test_a_read_that_holds_the_equals_sign_is_flagged_alone(gca, golden_dir, graph):
    reads = golden_reads(golden_dir)
    reads.insert(2, reads[1][:500] + "=" + reads[1][501:1000])
    ids = [b"r%d" % k for k in range(len(reads))]
    data = bm.stream([(i, bm.revcomp(r) if k % 2 else r, 0x10 if k % 2 else 0) for k, (i, r) in enumerate(zip(ids, reads))])
    fastq = b"".join(b"@" + i + b"\n" + r.encode() + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in zip(ids, reads))
    from_bam, bam_ids, _ = gca.ReadBatch.from_bam(data, header=True)
    from_fastq, fastq_ids, _ = gca.ReadBatch.from_text(fastq, "fastq")
    assert bam_ids == fastq_ids == ids and from_bam.blob == from_fastq.blob
    aligner = gca.Aligner(*graph, long_pass=True, keep_traces=True, keep_seeds=True, chain_traces=2)
    got = aligner.align_batch(from_bam, gaf_names=ids, other_formats=True)
    want = aligner.align_batch(from_fastq, gaf_names=ids, other_formats=True)
    assert [int(x) for x in np.asarray(got["failed_assertion"]) != 0] == [0, 0, 1, 0, 0, 0, 0]
    same_results(got, want)
    written = set(re.findall(rb"^(r\d+)\t", got["gaf"], flags=re.M))
    assert written and b"r2" not in written and written <= set(ids)
    from_bam.close()
    from_fastq.close()
