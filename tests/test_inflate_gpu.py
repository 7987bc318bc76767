"""The BGZF inflater on the device (csrc/hip/gc_inflate.hip) through every layer: gc_bgzf_inflate against Python's zlib on the blocks and refusals of
tests/test_inflate_host.py (which has shown the decoder bounded on them), this library's own deflate output reframed as BGZF, ReadBatch.from_bgzf against from_text,
and the command on a BGZF read file against the same reads as plain text and as ordinary gzip."""
import gzip
import os
import random
import struct
import sys
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bgzf_model as bm                            # noqa: E402
import test_inflate_host as host                   # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gca():
    import graphchainer_amd as g
    assert g.device_count() >= 1, "GPU tests need a device"
    return g


@pytest.fixture(scope="module")
def api(gca):
    from graphchainer_amd import api as a
    return a


def test_valid_blocks_equal_zlib(api):
    for name, data, f in host.valid_cases():
        text, consumed = api.bgzf_inflate(f)
        assert consumed == len(f), name
        assert text == data, name
    for name, data in bm.ACCEPTED_HANDMADE.items():                       # among them the match at distance 32 768, which no stream of zlib's holds
        blk = bm.handmade()[name][0]
        assert api.bgzf_inflate(blk) == (data, len(blk)), name


def test_files_of_several_blocks(api):
    text = host.fastq(5, 70, 7)[:900]
    three = bm.write(text, 300)
    assert len(three) > 28 and three.endswith(bm.EOF) and bm.bgzf_count(three) == 4
    assert api.bgzf_inflate(three) == (text, len(three))
    middle = bm.write(text[:300], 300, eof=False) + bm.EOF + bm.write(text[300:], 300)
    assert api.bgzf_inflate(middle) == (text, len(middle))
    whole = bm.write(text[:600], 300, eof=False)
    for cut in (1, 17, 18, 40, len(three) - len(whole) - 28 - 1):
        assert api.bgzf_inflate(three[:len(whole) + cut]) == (text[:600], len(whole)), cut
    assert api.bgzf_inflate(gzip.compress(text) + three) == (b"", 0)
    assert api.bgzf_inflate(b"") == (b"", 0)
    big = bm.frame(bm.deflate_raw(b"A" * 65537), zlib.crc32(b"A" * 65537), 65537)                # more text than a block holds: not BGZF, the walk stops
    assert api.bgzf_inflate(big) == (b"", 0) and api.bgzf_inflate(three + big) == (text, len(three))
    assert api.bgzf_inflate(three + gzip.compress(text)) == (text, len(three))          # an ordinary member further on stops the walk


def test_refusals_name_the_block_and_leave_the_device_usable(api):
    hand = bm.handmade()
    good_text = host.fastq(3, 60, 1)
    good = bm.block(good_text)
    for name in bm.GPU_REFUSALS:
        blk, verdict = hand[name]
        assert verdict is None
        with pytest.raises(api.BgzfError) as e:
            api.bgzf_inflate(good + blk + good)
        assert f"block 1 at byte {len(good)} " in str(e.value) and "error -1" in str(e.value), (name, str(e.value))
        assert api.bgzf_inflate(good + good) == (good_text + good_text, 2 * len(good)), name


def test_this_librarys_own_deflate_output_inflates(api):
    rng = random.Random(11)
    streams = [b"", b"a", host.fastq(4, 80, 9), bytes(rng.randrange(256) for _ in range(3000)), b"ACGT" * 5000, host.fastq(30, 500, 10)]
    for lz in (False, True):
        members = api.gzip_streams(streams, lz=lz)
        framed = b""
        for raw, member in zip(streams, members):
            assert member[:4] == b"\x1f\x8b\x08\x00" and gzip.decompress(member) == raw             # a plain 10-byte header, the deflate stream, CRC and ISIZE
            crc, isize = struct.unpack("<II", member[-8:])
            framed += bm.frame(member[10:-8], crc, isize)
        text, consumed = api.bgzf_inflate(framed)
        assert consumed == len(framed) and text == b"".join(streams), lz


def reads_text(fmt, seed):
    rng = random.Random(seed)
    reads = ["".join(rng.choice("ACGT") for _ in range(rng.randrange(50, 401))) for _ in range(40)]
    if fmt == "fastq":
        return "".join(f"@read{i} n={len(r)}\n{r}\n+\n{'I' * len(r)}\n" for i, r in enumerate(reads)).encode()
    return "".join(f">read{i} n={len(r)}\n" + "".join(r[k:k + 60] + "\n" for k in range(0, len(r), 60)) for i, r in enumerate(reads)).encode()


@pytest.mark.parametrize("fmt", ["fasta", "fastq"])
def test_from_bgzf_equals_from_text(api, fmt):
    text = reads_text(fmt, 21)
    want, want_ids, _ = api.ReadBatch.from_text(text, fmt)
    assert len(want_ids) == 40
    f = bm.write(text, 300)
    whole, ids, tail, consumed = api.ReadBatch.from_bgzf(b"", f, fmt, final=True)
    assert (ids, whole.blob, tail, consumed) == (want_ids, want.blob, b"", len(f))
    assert (whole.offsets == want.offsets).all() and (whole.lengths == want.lengths).all()
    assert whole.bgzf["blocks"] == bm.bgzf_count(f) and whole.bgzf["inflated_bytes"] == len(text)
    # in pieces of four blocks, the tail carried
    sizes = bm.bgzf_sizes(f)
    at, head, ids, blob, lengths = 0, b"", [], b"", []
    for k in range(0, len(sizes), 4):
        piece = f[at:at + sum(sizes[k:k + 4])]
        at += len(piece)
        batch, got, head, consumed = api.ReadBatch.from_bgzf(head, piece, fmt, final=k + 4 >= len(sizes))
        assert consumed == len(piece)
        ids += got
        blob += batch.blob
        lengths += [int(x) for x in batch.lengths]
        batch.close()
    assert at == len(f) and head == b""
    assert (ids, blob, lengths) == (want_ids, want.blob, [int(x) for x in want.lengths])
    whole.close()
    want.close()


def fastq_of(reads, ids):
    return b"".join(b"@" + i + b"\n" + r + b"\n+\n" + b"I" * len(r) + b"\n" for i, r in zip(ids, reads))


def test_the_command_on_a_bgzf_file(gca, api, golden_dir, tmp_path, capsys):
    from graphchainer_amd import cli
    gfa = os.path.join(golden_dir, "syn20k.gfa")
    reads = [l.strip().encode() for l in open(os.path.join(golden_dir, "syn20k.fa")) if not l.startswith(">")]
    text = fastq_of(reads, [b"r%d" % i for i in range(len(reads))])
    files = {"plain": ("reads.fq", text), "bgzf": ("reads.fq.gz", bm.write(text, 4000)), "gzip": ("reads.fq.gz", gzip.compress(text)),
             "appended": ("reads.fq.gz", bm.write(text[:9000], 4000, eof=False) + gzip.compress(text[9000:]))}
    gafs, blocks = {}, {}
    for kind, (name, data) in files.items():
        os.makedirs(tmp_path / kind)
        (tmp_path / kind / name).write_bytes(data)
        counts = cli.run(cli.resolve(["-g", gfa, "-f", str(tmp_path / kind / name), "-a", str(tmp_path / kind / "out.gaf"), "--batch-bytes", "20000"]))
        assert counts["reads"] == len(reads), kind
        gafs[kind], blocks[kind] = (tmp_path / kind / "out.gaf").read_bytes(), counts["bgzf_blocks"]
    assert len(gafs["plain"]) > 0 and gafs["bgzf"] == gafs["plain"] and gafs["gzip"] == gafs["plain"] and gafs["appended"] == gafs["plain"]
    assert blocks["plain"] == 0 and blocks["gzip"] == 0
    assert blocks["bgzf"] == bm.bgzf_count(files["bgzf"][1]) > 4 and blocks["appended"] == 3
    # one corrupt block: the line a bad gzip file gives, status 1, no output file
    good = files["bgzf"][1]
    sizes = bm.bgzf_sizes(good)
    at = sizes[0] + sizes[1] + 30
    os.makedirs(tmp_path / "bad")
    (tmp_path / "bad" / "reads.fq.gz").write_bytes(good[:at] + bytes([good[at] ^ 0x10]) + good[at + 1:])
    capsys.readouterr()
    status = cli.main(["-g", gfa, "-f", str(tmp_path / "bad" / "reads.fq.gz"), "-a", str(tmp_path / "bad" / "out.gaf"), "--batch-bytes", "20000"])
    err = capsys.readouterr().err
    assert status == 1 and "a gzipped read file could not be inflated" in err and "block 2" in err, err
    assert not (tmp_path / "bad" / "out.gaf").exists()
