"""python -m graphchainer_amd --corrected-out / --corrected-clipped-out on files, against the API's records for the same reads: input order across batches in flight, one
gzip member per record for a .gz name, the run without -a, and a GAF file that the new options leave as it was."""
import os
import subprocess
import sys
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden")


def command(*args):
    out = subprocess.run([sys.executable, "-m", "graphchainer_amd"] + [str(a) for a in args], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout + out.stderr
    return out


def gzip_members(data):
    """The inflated members of a file of concatenated gzip members, one by one."""
    members = []
    while data:
        d = zlib.decompressobj(16 + zlib.MAX_WBITS)
        members.append(d.decompress(data))
        assert d.eof
        data = d.unused_data
    return members


def test_the_two_files_across_batches_in_flight_and_without_alignments_out(tmp_path):
    import graphchainer_amd as gca
    assert gca.device_count() >= 1, "GPU tests need a device"
    gfa = os.path.join(GOLD, "syn20k.gfa")
    reads = [l.strip().encode() for l in open(os.path.join(GOLD, "syn20k.fa")) if not l.startswith(">")]
    reads.insert(2, b"A" * 400)                                               # a read without alignments: its lower-cased self
    ids = [b"r%d with words" % i for i in range(len(reads))]
    (tmp_path / "reads.fa").write_bytes(b"".join(b">" + i + b"\n" + r + b"\n" for i, r in zip(ids, reads)))
    # the API's records for the same reads, in one batch
    graph = gca.AlignmentGraph(gfa)
    batch = gca.ReadBatch(reads)
    out = gca.Aligner(graph, gca.MinimizerSeeder(graph), long_pass=True, device_output=1 | 8).align_batch(batch, gaf_names=ids, formats=("gaf", "corrected", "corrected_clipped"))
    split = lambda text, off: [text[int(off[k]):int(off[k + 1])] for k in range(len(off) - 1)]   # noqa: E731
    bodies, clipped = split(out["corrected"], out["corrected_rec_off"]), split(out["corrected_clipped"], out["corrected_clipped_rec_off"])
    assert len(bodies) == len(reads) and [b.split(b"\n")[0] for b in bodies] == [b">" + i for i in ids]
    assert bodies[2] == b">" + ids[2] + b"\n" + b"a" * 400 + b"\n" and len(clipped) >= len(reads) - 1

    plain = command("-g", gfa, "-f", tmp_path / "reads.fa", "-a", tmp_path / "plain.gaf", "--batch-bytes", 3000, "--inflight", 2)
    small = command("-g", gfa, "-f", tmp_path / "reads.fa", "-a", tmp_path / "o.gaf", "--corrected-out", tmp_path / "c.fa", "--corrected-clipped-out", tmp_path / "cc.fa.gz",
                    "--batch-bytes", 3000, "--inflight", 2)
    assert (tmp_path / "o.gaf").read_bytes() == (tmp_path / "plain.gaf").read_bytes() == out["gaf"]
    assert (tmp_path / "c.fa").read_bytes() == out["corrected"]
    assert gzip_members((tmp_path / "cc.fa.gz").read_bytes()) == clipped       # one member per record, in input order
    assert not [p for p in os.listdir(tmp_path) if ".tmp" in p]
    # three batches or more: 3000 bytes of file text hold one read of the seven
    assert sum(len(r) for r in reads) > 3 * 3000

    command("-g", gfa, "-f", tmp_path / "reads.fa", "--corrected-out", tmp_path / "only.fasta.gz", "--corrected-clipped-out", tmp_path / "only_clipped.fasta",
            "--batch-bytes", 3000, "--inflight", 2)
    assert gzip_members((tmp_path / "only.fasta.gz").read_bytes()) == bodies
    assert (tmp_path / "only_clipped.fasta").read_bytes() == out["corrected_clipped"]
    del plain, small
