"""python -m graphchainer_amd -f reads.bam: tests/golden/syn20k.fa's reads written as unaligned BAM by tests/bam_model.py give, byte for byte, what the same command gives
on syn20k.fa - with the defaults, with pieces so small that records span them, and beside a .fa in one -f list."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bam_model as bm                             # noqa: E402
import fastx_model as fm                           # noqa: E402

pytestmark = pytest.mark.gpu


def command(*args):
    out = subprocess.run([sys.executable, "-m", "graphchainer_amd"] + [str(a) for a in args], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout + out.stderr
    return out


def strip(text):
    return [line.split(b"\t", 1)[1] for line in text.splitlines()]


def test_a_bam_file_gives_what_the_fasta_file_gives(golden_dir, tmp_path):
    import graphchainer_amd as g
    assert g.device_count() >= 1, "GPU tests need a device"
    gfa, fa = os.path.join(golden_dir, "syn20k.gfa"), os.path.join(golden_dir, "syn20k.fa")
    ids, reads, _ = fm.parse(open(fa, "rb").read(), "fasta")
    records = []
    for k, (i, r) in enumerate(zip(ids, reads)):
        r = r.decode()
        records.append((i, bm.revcomp(r) if k % 2 else r, 0x10 if k % 2 else 4, (), b"RGZa\x00"))
        if k == 2:
            records.append((i, r[:100], 0x900))                                   # a supplementary secondary record of the same read: left out
    bam = tmp_path / "reads.bam"
    bam.write_bytes(bm.write(records, block_sizes=(4000,)))
    command("-g", gfa, "-f", fa, "-a", tmp_path / "fa.gaf")
    want = (tmp_path / "fa.gaf").read_bytes()
    assert strip(want) == strip(open(os.path.join(golden_dir, "syn20k.expected.gaf"), "rb").read()) and len(want.splitlines()) >= 6

    out = command("-g", gfa, "-f", bam, "-a", tmp_path / "bam.gaf")
    assert (tmp_path / "bam.gaf").read_bytes() == want
    assert "1 BAM records were left out" in out.stderr
    command("-g", gfa, "-f", bam, "-a", tmp_path / "small.gaf", "--batch-bytes", 20000, "--inflight", 2)       # (the whole file is one piece of 19 kB)
    assert (tmp_path / "small.gaf").read_bytes() == want
    command("-g", gfa, "-f", bam, "-a", tmp_path / "tiny.gaf", "--batch-bytes", 3000)                           # one BGZF block of 4 000 bytes per piece: every record spans two
    assert (tmp_path / "tiny.gaf").read_bytes() == want
    command("-g", gfa, "-f", fa, bam, "-a", tmp_path / "both.gaf")                                               # a .fa and a .bam in one -f list
    assert (tmp_path / "both.gaf").read_bytes() == want + want
    assert sorted(p.name for p in tmp_path.iterdir()) == ["bam.gaf", "both.gaf", "fa.gaf", "reads.bam", "small.gaf", "tiny.gaf"]     # no temporary file stays
