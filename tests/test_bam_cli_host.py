"""What a .bam read file adds to the command line's host half, without a GPU: the format by file name, the batch count, file_pieces on a file from tests/bam_model.py under
both bgzf settings, and parse_pieces' header flag, with the parser stubbed out."""
import os
import sys
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bam_model as bm                             # noqa: E402
import bgzf_model                                  # noqa: E402
from graphchainer_amd import api, cli              # noqa: E402

RECORDS = [(b"r%d" % k, "ACGTTGCA" * (k + 1), 0x10 if k % 3 == 0 else 4, (), b"RGZx\x00") for k in range(40)]


def test_the_format_by_file_name():
    assert api.fastx_file_format("x.bam") == ("bam", True) and api.fastx_file_format(b"dir.fa/reads.bam") == ("bam", True)
    assert api.fastx_file_format("x.BAM") == (None, False)
    assert api.fastx_file_format("x.bam.gz") == (None, True)
    assert api.fastx_file_format(".bam") == (None, False)                    # a name is longer than its suffix, as for the other formats
    assert api.fastx_file_format("bam.fa") == ("fasta", False) and api.fastx_file_format("x.fq.gz") == ("fastq", True)
    assert "unaligned bam" in cli.HELP.split("--reads")[1].split("\n")[0]


def test_choose_inflight_counts_two_bases_per_three_bytes_of_bam():
    assert cli.FILE_BYTES_PER_READ_BASE["bam"] == 1.5
    free, batch = cli.LONG_SCRATCH_BYTES + 100 * 10 ** 9, 150 << 20
    want = (free - cli.LONG_SCRATCH_BYTES) // ((batch * 2 // 3) * cli.BATCH_BYTES_PER_READ_BASE)
    assert 1 < want < cli.MAX_INFLIGHT
    assert cli.choose_inflight(64, free, batch, "bam") == want
    assert cli.choose_inflight(64, free, batch, "fasta") <= want <= cli.choose_inflight(64, free, batch, "fastq")
    assert cli.choose_inflight(64, free, batch * 3 // 2, "bam") == cli.choose_inflight(64, free, batch, "fasta")
    assert cli.choose_inflight(3, free, batch, "bam") == 1 and cli.choose_inflight(64, 0, batch, "bam") == 1
    assert min(("fastq", "bam"), key=cli.FILE_BYTES_PER_READ_BASE.get) == "bam" and min(("fastq", "bam", "fasta"), key=cli.FILE_BYTES_PER_READ_BASE.get) == "fasta"


@pytest.mark.parametrize("eof", [True, False])
def test_file_pieces_on_a_bam_file_under_both_settings(tmp_path, eof):
    stream = bm.stream(RECORDS)
    path = tmp_path / "reads.bam"
    path.write_bytes(bm.bgzf(stream, (300,), eof=eof))
    host = list(api.file_pieces([str(path)], batch_bytes=1000, bgzf="host"))
    assert len(host) > 3 and [last for _, _, last in host] == [False] * (len(host) - 1) + [True] and {fmt for fmt, _, _ in host} == {"bam"}
    assert not any(isinstance(piece, api.BgzfPiece) for _, piece, _ in host) and b"".join(piece for _, piece, _ in host) == stream
    device = list(api.file_pieces([str(path)], batch_bytes=1000, bgzf="device"))
    assert len(device) > 3 and [last for _, _, last in device] == [False] * (len(device) - 1) + [True] and {fmt for fmt, _, _ in device} == {"bam"}
    assert all(isinstance(piece, api.BgzfPiece) for _, piece, _ in device)
    assert b"".join(piece for _, piece, _ in device) == path.read_bytes()                     # every block goes up, the end-of-file block with the last piece
    assert sum(piece.text_bytes for _, piece, _ in device) == len(stream)
    assert device[-1][1].endswith(bgzf_model.EOF) == eof
    assert b"".join(zlib.decompress(bytes(piece)[at:at + size], 31) for _, piece, _ in device
                    for at, size in zip(_starts(bytes(piece)), bgzf_model.bgzf_sizes(bytes(piece)))) == stream


def _starts(data):
    at, out = 0, []
    for size in bgzf_model.bgzf_sizes(data):
        out.append(at)
        at += size
    return out


class FakeBatch:
    def __init__(self, inflated=0):
        self.bam = {"skipped": 2}
        self.bgzf = {"blocks": 1, "inflated_bytes": inflated}

    def close(self):
        pass


def test_parse_pieces_sets_the_header_flag_at_the_start_of_every_file(monkeypatch):
    calls = []

    def from_bam(data, header, final=True):
        consumed = len(data) if final else 0 if len(data) < 5 else len(data) - 2               # fewer than 5 bytes: not even the header is whole
        calls.append(("bam", bytes(data), header, final))
        return FakeBatch(), [b"id"] if consumed else [], consumed

    def from_bam_bgzf(head, data, header, final=True):
        text = bytes(head) + bytes(data).upper()                                              # "inflating" is upper-casing here
        consumed = len(text) if final else 0 if len(text) < 5 else len(text) - 2
        calls.append(("bgzf", bytes(head), bytes(data), header, final))
        return FakeBatch(len(data)), [b"id"] if consumed else [], text[consumed:], len(data)

    def from_text(data, fmt, final=True):
        calls.append(("text", bytes(data), fmt, final))
        return FakeBatch(), [b"id"], len(data)

    monkeypatch.setattr(api.ReadBatch, "from_bam", staticmethod(from_bam))
    monkeypatch.setattr(api.ReadBatch, "from_bam_bgzf", staticmethod(from_bam_bgzf))
    monkeypatch.setattr(api.ReadBatch, "from_text", staticmethod(from_text))

    def piece(text):
        p = api.BgzfPiece(text)
        p.text_bytes = len(text)
        return p

    pieces = [("bam", b"abc", False), ("bam", b"defg", False), ("bam", b"hi", True),            # file 1: the first call consumes nothing, so the second still expects the header
              ("bam", piece(b"jk"), False), ("bam", piece(b"lmnop"), False), ("bam", piece(b"q"), True),   # file 2, compressed pieces
              ("fasta", b">x\nA\n", True),
              ("bam", b"rstuvw", True)]                                                        # file 4: one piece
    counts = {}
    out = list(api.parse_pieces(iter(pieces), counts=counts))
    assert calls == [("bam", b"abc", True, False), ("bam", b"abcdefg", True, False), ("bam", b"fghi", False, True),
                     ("bgzf", b"", b"jk", True, False), ("bgzf", b"JK", b"lmnop", True, False), ("bgzf", b"OP", b"q", False, True),
                     ("text", b">x\nA\n", "fasta", True),
                     ("bam", b"rstuvw", True, True)]
    assert len(out) == 6 and counts["bam_skipped"] == 14 and counts["bgzf_blocks"] == 3
