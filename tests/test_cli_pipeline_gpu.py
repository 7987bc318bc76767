"""python -m graphchainer_amd with several batches in flight (--inflight) and several replicas (--devices): the same files as with one batch at a time, whatever order the
workers finish in. The reads are the six golden reads, or those four times over under distinct ids, cut by --batch-bytes 3000 into more batches than there are workers."""
import gzip
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_cli_gpu import R_IDS, fasta, fastq, gam_messages, gca, golden, yardstick      # noqa: E402,F401 - gca and golden are that module's fixtures, used here as they are

pytestmark = pytest.mark.gpu

FORMATS = ("gaf", "json", "gam")
SMALL = ("--batch-bytes", 3000)


def command(*args, status=0):
    out = subprocess.run([sys.executable, "-m", "graphchainer_amd"] + [str(a) for a in args], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == status, out.stdout + out.stderr
    return out


def outputs(directory, stem):
    paths = {f: directory / f"{stem}.{f}" for f in FORMATS}
    return paths, [x for f in FORMATS for x in ("-a", paths[f])]


def same_files(got, want):
    assert got["gaf"].read_bytes() == want["gaf"].read_bytes() and got["json"].read_bytes() == want["json"].read_bytes()
    assert gzip.decompress(got["gam"].read_bytes()) == gzip.decompress(want["gam"].read_bytes())
    assert want["gaf"].read_bytes().count(b"\n") >= 5


def four_times(reads):
    """24 reads: the six golden ones four times, every copy under an id of its own."""
    return [r for _ in range(4) for r in reads], [b"c%d_r%d" % (c, i) for c in range(4) for i in range(len(reads))]


def test_three_writers_with_three_batches_in_flight(golden, golden_dir, tmp_path):
    gfa, reads, _, _ = golden
    (tmp_path / "reads.fa").write_bytes(fasta(reads, R_IDS))
    three, three_args = outputs(tmp_path, "three")
    one, one_args = outputs(tmp_path, "one")
    command("-g", gfa, "-f", tmp_path / "reads.fa", *three_args, "--inflight", 3, *SMALL)
    command("-g", gfa, "-f", tmp_path / "reads.fa", *one_args, "--inflight", 1, *SMALL)
    expected = lambda suffix: open(os.path.join(golden_dir, "syn20k.expected." + suffix), "rb").read()   # noqa: E731
    assert three["gaf"].read_bytes() == expected("gaf") and three["json"].read_bytes() == expected("json")
    assert gzip.decompress(three["gam"].read_bytes()) == gzip.decompress(one["gam"].read_bytes())
    assert gam_messages(three["gam"].read_bytes()) == gam_messages(gzip.compress(expected("gam")))
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(["reads.fa"] + [p.name for p in three.values()] + [p.name for p in one.values()])     # no temporary file stays


def test_24_reads_over_two_files_with_four_batches_in_flight(gca, golden, tmp_path):
    gfa, reads, _, _ = golden
    many, ids = four_times(reads)
    paths = [tmp_path / "first.fq", tmp_path / "second.fa.gz"]
    paths[0].write_bytes(fastq(many[:11], ids[:11]))
    text = fasta(many[11:], ids[11:], 70)
    paths[1].write_bytes(gzip.compress(text[:9000]) + gzip.compress(text[9000:]))
    four, four_args = outputs(tmp_path, "four")
    one, one_args = outputs(tmp_path, "one")
    command("-g", gfa, "-f", *paths, *four_args, "--inflight", 4, *SMALL)
    command("-g", gfa, "-f", *paths, *one_args, "--inflight", 1, *SMALL)
    same_files(four, one)
    want = yardstick(gca, golden, [str(p) for p in paths])
    assert want["gaf"].count(b"\n") >= 20
    assert four["gaf"].read_bytes() == want["gaf"]


def test_two_replicas_on_one_device(gca, golden, tmp_path):
    from graphchainer_amd import cli
    gfa, reads, _, _ = golden
    many, ids = four_times(reads)
    (tmp_path / "reads.fq").write_bytes(fastq(many, ids))
    two, two_args = outputs(tmp_path, "two")
    single, single_args = outputs(tmp_path, "single")
    command("-g", gfa, "-f", tmp_path / "reads.fq", *two_args, "--devices", "0,0", "--inflight", 2, *SMALL)
    command("-g", gfa, "-f", tmp_path / "reads.fq", *single_args, "--inflight", 2, *SMALL)
    same_files(two, single)
    # in this process, for what run() reports
    inside, inside_args = outputs(tmp_path, "inside")
    counts = cli.run(cli.resolve(["-g", gfa, "-f", str(tmp_path / "reads.fq")] + [str(a) for a in inside_args] + ["--devices", "0,0", "--inflight", "2", "--batch-bytes", "3000"]))
    same_files(inside, single)
    assert counts["reads"] == 24 and counts["devices"] == [0, 0] and counts["inflight"] == 2 and counts["retired_workers"] == 0
    assert counts["batches"] > 4, "no more batches than workers: nothing is reused"
    assert len(counts["batches_per_replica"]) == 2 and min(counts["batches_per_replica"]) >= 1 and sum(counts["batches_per_replica"]) == counts["batches"]
    assert len(counts["setup_seconds"]) == 2 and all(s > 0 for s in counts["setup_seconds"])
    assert set(counts["stage_seconds"]) == {"read", "parse", "align", "write"}
    assert all(set(stage) == {"busy", "waiting_in", "waiting_out"} for stage in counts["stage_seconds"].values()) and counts["stage_seconds"]["align"]["busy"] > 0
    for key in ("flagged", "failed_assertion", "capacity_exceeded", "seconds"):
        assert key in counts
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(["reads.fq"] + [p.name for group in (two, single, inside) for p in group.values()])


def test_mem_seeds_with_three_batches_in_flight(golden, tmp_path):
    gfa, reads, _, _ = golden
    many, ids = four_times(reads)
    (tmp_path / "reads.fa").write_bytes(fasta(many, ids))
    seeder = ("--seeds-minimizer-density", 0, "--seeds-mem-count", 100)
    three, three_args = outputs(tmp_path, "three")
    one, one_args = outputs(tmp_path, "one")
    command("-g", gfa, "-f", tmp_path / "reads.fa", *three_args, *seeder, "--inflight", 3, *SMALL)
    command("-g", gfa, "-f", tmp_path / "reads.fa", *one_args, *seeder, "--inflight", 1, *SMALL)
    same_files(three, one)


def test_a_letter_outside_the_alphabet_with_three_batches_in_flight(gca, golden, tmp_path):
    gfa, reads, _, _ = golden
    bad = reads[2][:700] + b"!" + reads[2][701:]
    (tmp_path / "reads.fa").write_bytes(fasta(reads[:2] + [bad] + reads[3:], R_IDS))
    out = command("-g", gfa, "-f", tmp_path / "reads.fa", "-a", tmp_path / "out.gaf", "--inflight", 3, *SMALL)
    assert "1 of 6 reads were flagged" in out.stderr
    lines = (tmp_path / "out.gaf").read_bytes().splitlines()
    assert sorted({l.split(b"\t")[0] for l in lines}) == [b"r0", b"r1", b"r3", b"r4", b"r5"]
    (tmp_path / "good.fa").write_bytes(fasta(reads[:2] + reads[3:], R_IDS[:2] + R_IDS[3:]))
    assert (tmp_path / "out.gaf").read_bytes() == yardstick(gca, golden, [str(tmp_path / "good.fa")])["gaf"]


def test_a_missing_second_file_ends_the_run_with_no_output(golden, tmp_path):
    gfa, reads, _, _ = golden
    many, ids = four_times(reads)
    (tmp_path / "good.fa").write_bytes(fasta(many, ids))
    paths, args = outputs(tmp_path, "out")
    out = command("-g", gfa, "-f", tmp_path / "good.fa", tmp_path / "missing.fa", *args, "--inflight", 3, *SMALL, status=1)
    # (the library's own note about a preset GPU_MAX_HW_QUEUES below 8, which it prints when a second stream is made, is not the command's message)
    lines = [line for line in out.stderr.splitlines() if not line.startswith("[graphchainer_amd] note: GPU_MAX_HW_QUEUES")]
    assert len(lines) == 1 and "missing.fa" in lines[0]
    assert sorted(p.name for p in tmp_path.iterdir()) == ["good.fa"]      # no output file and no temporary file
