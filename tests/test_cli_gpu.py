"""python -m graphchainer_amd on files, against the entry points it is plumbing over: Aligner(...).align_batch(ReadBatch(reads), gaf_names=ids, formats=...) with the
parameters the command line stands for, the reads and ids being what tests/fastx_model.py reads from the same files."""
import gzip
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fastx_model as fm                           # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gca():
    import graphchainer_amd as g
    assert g.device_count() >= 1, "GPU tests need a device"
    return g


@pytest.fixture(scope="module")
def golden(gca, golden_dir):
    gfa = os.path.join(golden_dir, "syn20k.gfa")
    reads = [l.strip().encode() for l in open(os.path.join(golden_dir, "syn20k.fa")) if not l.startswith(">")]
    graph = gca.AlignmentGraph(gfa)
    return gfa, reads, graph, gca.MinimizerSeeder(graph)


def fasta(reads, ids, width=60):
    return b"".join(b">" + i + b"\n" + b"".join(r[k:k + width] + b"\n" for k in range(0, len(r), width)) for i, r in zip(ids, reads))


def fastq(reads, ids):
    return b"".join(b"@" + i + b"\n" + r + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in zip(ids, reads))


def command(*args):
    out = subprocess.run([sys.executable, "-m", "graphchainer_amd"] + [str(a) for a in args], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout + out.stderr
    return out


def yardstick(gca, golden, paths, formats=("gaf",), merge=False, seeds=None, **kw):
    """The code before the command line existed, on what the model reads from the files."""
    _, _, graph, seeder = golden
    ids, reads = [], []
    for path in paths:
        fmt, gz = fm.file_format(path)
        data = open(path, "rb").read()
        i, r, _ = fm.parse(gzip.decompress(data) if gz else data, fmt)
        ids += i
        reads += r
    batch = gca.ReadBatch(reads)
    aligner = gca.Aligner(graph, None if seeds else seeder, long_pass=True, keep_traces=2, **kw)
    seed_batch = gca.MxmIndex(graph).seeds(batch, seeds[0], count=seeds[1], min_len=seeds[2]) if seeds else None
    return aligner.align_batch(batch, seeds=seed_batch, gaf_names=ids, formats=formats, cigar_match_mismatch_merge=merge)


R_IDS = [b"r%d" % i for i in range(6)]


def gam_messages(gam):
    """The GAM file's messages in order, out of their groups (varint count, then varint size + message each): a group never spans two batches, so the groups follow the
    batches while the messages do not."""
    from vg_descriptor import read_varint
    raw, at, messages = gzip.decompress(gam), 0, []
    while at < len(raw):
        count, at = read_varint(raw, at)
        for _ in range(count):
            size, at = read_varint(raw, at)
            messages.append(raw[at:at + size])
            at += size
    assert at == len(raw)
    return messages


def test_three_writers_equal_the_golden_files(gca, golden, golden_dir, tmp_path):
    gfa, reads, _, _ = golden
    (tmp_path / "reads.fa").write_bytes(fasta(reads, R_IDS))
    outs = [tmp_path / "out.gaf", tmp_path / "out.json", tmp_path / "out.gam"]
    command("-g", gfa, "-f", tmp_path / "reads.fa", "-a", outs[0], "-a", outs[1], "-a", outs[2])
    expected = lambda suffix: open(os.path.join(golden_dir, "syn20k.expected." + suffix), "rb").read()   # noqa: E731
    assert outs[0].read_bytes() == expected("gaf")
    assert outs[1].read_bytes() == expected("json")
    assert gzip.decompress(outs[2].read_bytes()) == expected("gam")      # (the golden file is the inflated stream itself)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["out.gaf", "out.gam", "out.json", "reads.fa"]     # no temporary file stays
    # a smaller chunk of file text per batch: the same three files
    small = [tmp_path / "small.gaf", tmp_path / "small.json", tmp_path / "small.gam"]
    command("-g", gfa, "-f", tmp_path / "reads.fa", "-a", small[0], "-a", small[1], "-a", small[2], "--batch-bytes", 3000)
    assert small[0].read_bytes() == expected("gaf") and small[1].read_bytes() == expected("json")
    assert gam_messages(small[2].read_bytes()) == gam_messages(outs[2].read_bytes()) and len(gam_messages(outs[2].read_bytes())) >= 6


def test_the_golden_reads_file_as_it_is(gca, golden, golden_dir, tmp_path):
    """The ids of tests/golden/syn20k.fa are its own: the lines equal the golden file's but for the first column."""
    gfa = golden[0]
    command("-g", gfa, "-f", os.path.join(golden_dir, "syn20k.fa"), "-a", tmp_path / "x.gaf")
    strip = lambda text: [l.split(b"\t", 1)[1] for l in text.splitlines()]   # noqa: E731
    assert strip((tmp_path / "x.gaf").read_bytes()) == strip(open(os.path.join(golden_dir, "syn20k.expected.gaf"), "rb").read())
    assert (tmp_path / "x.gaf").read_bytes() == yardstick(gca, golden, [os.path.join(golden_dir, "syn20k.fa")])["gaf"]


@pytest.mark.parametrize("kind", ["fq", "fa.gz", "fq.gz", "two files", "descriptions"])
def test_other_files_equal_the_yardstick(gca, golden, tmp_path, kind):
    gfa, reads, _, _ = golden
    if kind == "two files":
        paths = [tmp_path / "first.fq", tmp_path / "second.fa.gz"]
        paths[0].write_bytes(fastq(reads[:3], R_IDS[:3]))
        paths[1].write_bytes(gzip.compress(fasta(reads[3:], R_IDS[3:], 70)[:-1]))     # (no newline at the end: the last line of a FASTA file is lost, here as in the reference)
    elif kind == "descriptions":
        paths = [tmp_path / "described.fq"]
        paths[0].write_bytes(fastq(reads, [b"r%d length=%d\tstrand +  " % (i, len(r)) for i, r in enumerate(reads)]).replace(b"\n", b"\r\n"))
    else:
        paths = [tmp_path / ("reads." + kind)]
        data = fastq(reads, R_IDS) if kind.startswith("fq") else fasta(reads, R_IDS, 80)
        paths[0].write_bytes(gzip.compress(data[:5000]) + gzip.compress(data[5000:]) if kind.endswith(".gz") else data)
    formats = ("gaf", "json", "gam")
    outs = {f: tmp_path / ("out." + f) for f in formats}
    command("-g", gfa, "-f", *paths, *[x for f in formats for x in ("-a", outs[f])])
    want = yardstick(gca, golden, [str(p) for p in paths], formats)
    assert want["gaf"].count(b"\n") >= 5
    assert outs["gaf"].read_bytes() == want["gaf"] and outs["json"].read_bytes() == want["json"]
    assert gam_messages(outs["gam"].read_bytes()) == gam_messages(want["gam"]) and len(gam_messages(want["gam"])) >= 5


MODES = [
    (["--no-colinear-chaining", "--greedy-length"], dict(colinear_chaining=False, selection_method=0), {}),
    (["--no-colinear-chaining", "--all-alignments"], dict(colinear_chaining=False, selection_method=7), {}),
    (["--no-colinear-chaining", "--try-all-seeds", "--seeds-extend-density", "0.002"], dict(colinear_chaining=False, selection_method=0, seed_extend_density=-1.0), {}),
    (["--no-colinear-chaining", "--seeds-extend-density", "0.002"], dict(colinear_chaining=False, selection_method=0, seed_extend_density=0.002), {}),
    (["--fast-mode"], dict(fast_mode=True), {}),
    (["--precise-clipping", "0.66"], dict(precise_clipping=0.66), {}),
    (["--cigar-match-mismatch"], {}, dict(merge=True)),
    (["--seeds-minimizer-density", "0", "--seeds-mem-count", "100"], dict(seed_density=0.0), dict(seeds=("mem", 100, 20))),
]


@pytest.mark.parametrize("mode", MODES, ids=[" ".join(m[0]) for m in MODES])
def test_modes_equal_the_yardstick_with_the_same_parameters(gca, golden, tmp_path, mode):
    args, params, other = mode
    gfa, reads, _, _ = golden
    (tmp_path / "reads.fq").write_bytes(fastq(reads, R_IDS))
    command("-g", gfa, "-f", tmp_path / "reads.fq", "-a", tmp_path / "out.gaf", *args)
    want = yardstick(gca, golden, [str(tmp_path / "reads.fq")], **params, **other)
    assert want["gaf"].count(b"\n") >= 4
    assert (tmp_path / "out.gaf").read_bytes() == want["gaf"]


def test_a_read_with_a_letter_outside_the_alphabet_is_reported_and_skipped(gca, golden, tmp_path):
    gfa, reads, _, _ = golden
    bad = reads[2][:700] + b"!" + reads[2][701:]
    (tmp_path / "reads.fa").write_bytes(fasta(reads[:2] + [bad] + reads[3:], R_IDS))
    out = command("-g", gfa, "-f", tmp_path / "reads.fa", "-a", tmp_path / "out.gaf")
    assert "1 of 6 reads were flagged" in out.stderr
    lines = (tmp_path / "out.gaf").read_bytes().splitlines()
    assert sorted({l.split(b"\t")[0] for l in lines}) == [b"r0", b"r1", b"r3", b"r4", b"r5"]
    (tmp_path / "good.fa").write_bytes(fasta(reads[:2] + reads[3:], R_IDS[:2] + R_IDS[3:]))
    assert (tmp_path / "out.gaf").read_bytes() == yardstick(gca, golden, [str(tmp_path / "good.fa")])["gaf"]


def test_index_cache_is_saved_by_the_first_run_and_loaded_by_the_second(gca, golden, golden_dir, tmp_path):
    """--index-cache FILE: the first run builds graph and minimizer index and saves them, the second loads them; both write the golden lines. A file with another
    minimizer length is refused with one line."""
    gfa, reads, _, _ = golden
    (tmp_path / "reads.fa").write_bytes(fasta(reads, R_IDS))
    cache = tmp_path / "index.gcidx"
    expected = open(os.path.join(golden_dir, "syn20k.expected.gaf"), "rb").read()
    command("-g", gfa, "-f", tmp_path / "reads.fa", "-a", tmp_path / "first.gaf", "--index-cache", cache)
    assert cache.exists() and (tmp_path / "first.gaf").read_bytes() == expected
    info = gca.api.check_index_cache(str(cache))
    assert info["has_seeder"] and (info["k"], info["w"]) == (15, 20)
    command("-g", tmp_path / "the graph is not read again.gfa", "-f", tmp_path / "reads.fa", "-a", tmp_path / "second.gaf", "--index-cache", cache)     # (an existing file wins)
    assert (tmp_path / "second.gaf").read_bytes() == expected
    out = subprocess.run([sys.executable, "-m", "graphchainer_amd", "-g", gfa, "-f", str(tmp_path / "reads.fa"), "-a", str(tmp_path / "third.gaf"), "--index-cache", str(cache),
                          "--seeds-minimizer-length", "13"], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 1 and "holds no minimizer index of length 13" in out.stderr and len(out.stderr.splitlines()) == 1
    assert not (tmp_path / "third.gaf").exists()
