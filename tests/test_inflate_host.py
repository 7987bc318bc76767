"""The BGZF inflater without a GPU: the per-block decoder every wave of k_bgzf_inflate runs (csrc/hip/gc_inflate_core.hpp) built with g++ into an ordinary program
(tests/inflate_host/inflate_host_test.cpp), once as it is and once more with -fsanitize=address,undefined, and held to Python's zlib: on valid blocks of every kind, on every
single-bit flip of four small blocks, and on deflate streams made by hand for each refusal. Then file_pieces' bgzf keyword, which needs neither library nor device."""
import gzip
import os
import random
import subprocess
import sys
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bgzf_model as bm                            # noqa: E402
from graphchainer_amd import api                   # noqa: E402

COMPRESSIONS = {"stored": dict(level=0), "fixed": dict(strategy=zlib.Z_FIXED), "default": dict(), "memlevel 1": dict(mem=1), "level 9": dict(level=9)}


def fastq(n_reads, length, seed):
    rng = random.Random(seed)
    return "".join(f"@read{i} len={length}\n{''.join(rng.choice('ACGT') for _ in range(length))}\n+\n{''.join(chr(33 + rng.randrange(40)) for _ in range(length))}\n" for i in range(n_reads)).encode()


def valid_inputs():
    rng = random.Random(5)
    half = bm.MAX_DISTANCE_HALF
    return {"empty": b"", "one byte": b"x", "three records": fastq(3, 60, 1), "65280 of fastq": fastq(40, 900, 2)[:65280], "65536 A": b"A" * 65536,
            "32768 random twice": half + half, "60000 random": bytes(rng.randrange(256) for _ in range(60000))}


def valid_cases():
    """(name, text, file). Where the deflate stream of the text does not fit one block of 64 KiB the writer halves the text: HALVED names those cases. The one that matters,
    "32768 random twice", never holds a match that way (and zlib's deflate stops 262 short of distance 32 768 anyway): bm.max_distance_stream() is that text in one block."""
    return [(f"{i} / {c}", data, bm.write(data, 65536, eof=False, **kw) if data else bm.EOF) for i, data in valid_inputs().items() for c, kw in COMPRESSIONS.items()]


HALVED = {"65536 A / stored"} | {f"32768 random twice / {c}" for c in COMPRESSIONS}


def mutation_blocks():
    text = fastq(3, 60, 3)
    return [bm.block(text, **kw) for kw in (COMPRESSIONS["stored"], COMPRESSIONS["fixed"], COMPRESSIONS["default"], COMPRESSIONS["memlevel 1"])]


def mutations():
    return [blk[:byte] + bytes([blk[byte] ^ (1 << bit)]) + blk[byte + 1:] for blk in mutation_blocks() for byte in range(18, len(blk)) for bit in range(8)]


@pytest.fixture(scope="module")
def corpus():
    """(file, what zlib gives or None)"""
    cases = [(f, data) for _, data, f in valid_cases()]
    cases += [(m, bm.zlib_verdict(m)) for m in mutations()]
    cases += list(bm.handmade().values())
    return cases


def _build(tmp, sanitize):
    out = str(tmp / ("inflate_host_test_san" if sanitize else "inflate_host_test"))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "graphchainer_amd", "csrc", "hip"),
                    os.path.join(ROOT, "tests", "inflate_host", "inflate_host_test.cpp"), "-o", out] + flags, check=True, timeout=600)
    return out


def _run(exe, tmp, corpus):
    path = str(tmp / "cases.txt")
    with open(path, "w") as f:
        for member, _ in corpus:
            f.write((member.hex() or "-") + "\n")
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.split("\n")
    assert len(lines) == len(corpus) + 1
    statuses = []
    for k, ((member, want), line) in enumerate(zip(corpus, lines)):
        word = line.split(" ")
        if want is None and api.bgzf_member(member) is None:      # an ISIZE above 64 KiB: not a BGZF block, so the member is left to zlib - which refuses it
            assert line == "OK 0 -", (k, line[:80], member[:64].hex())
            statuses.append(-1)
        elif want is None:
            assert word[0] == "ERR" and word[1] == "0", (k, line[:80], member[:64].hex())
            statuses.append(int(word[2]))
        else:
            assert word[0] == "OK" and int(word[1]) == len(member), (k, line[:80], member[:64].hex())
            assert (b"" if word[2] == "-" else bytes.fromhex(word[2])) == want, (k, member[:64].hex())
            statuses.append(0)
    return statuses


def test_the_cases_cover_what_they_claim(corpus):
    for name, data, f in valid_cases():
        assert gzip.decompress(f + bm.EOF) == data, name
    kinds = set()
    for name, data, f in valid_cases():
        first = f[18] >> 1 & 3                                     # the type of the block's first deflate block
        kinds.add(first)
    assert kinds == {0, 1, 2}
    assert {name for name, _, f in valid_cases() if bm.bgzf_count(f) > 1} == HALVED and all(bm.bgzf_count(f) <= 2 for _, _, f in valid_cases())
    assert any(bm.bgzf_sizes(f) == [len(f)] and f[-4:] == (65536).to_bytes(4, "little") for name, _, f in valid_cases() if name.startswith("65536 A"))   # ISIZE at its maximum
    far = bm.handmade()["distance 32768"][0]                              # one block of ISIZE 65 536 whose second half is matches at distance 32 768
    assert bm.bgzf_sizes(far) == [len(far)] and far[-4:] == (65536).to_bytes(4, "little") and len(bm.cdata_of(far)) < 32768 + 600
    assert bm.zlib_verdict(far) == valid_inputs()["32768 random twice"] == bm.MAX_DISTANCE_HALF * 2
    muts = [(m, bm.zlib_verdict(m)) for m in mutations()]
    assert 8000 < len(muts) < 12000
    accepted = [(m, got) for m, got in muts if got is not None]
    assert 0 < len(accepted) < 40 and all(got == fastq(3, 60, 3) for _, got in accepted)   # padding bits: zlib returns the original bytes
    hand = bm.handmade()
    assert {name for name, (_, got) in hand.items() if got is not None} == set(bm.ACCEPTED_HANDMADE)
    assert all(hand[name][1] == text for name, text in bm.ACCEPTED_HANDMADE.items())
    assert set(bm.GPU_REFUSALS) <= set(hand)
    # memLevel 1 gives many dynamic blocks in one BGZF block
    d = zlib.decompressobj(-15)
    blk = bm.block(valid_inputs()["65280 of fastq"], mem=1)
    assert len(blk) < 65536 and d.decompress(bm.cdata_of(blk)) == valid_inputs()["65280 of fastq"]


# InfStatus (csrc/hip/gc_inflate_core.hpp) of every stream made by hand: each is refused for the reason it was made for
HANDMADE_STATUS = {"crc bit": 15, "isize bit": 12, "stream past the data": 13, "stream ends early": 14, "block type 3": 1, "stored len nlen": 2, "hlit 287": 3, "hdist 31": 3,
                   "repeat 16 first": 4, "repeat past the end": 5, "no end code": 6, "over-subscribed": 7, "incomplete": 8, "incomplete code-length code": 8,
                   "single distance code": 0, "distance 32768": 0, "the other bit of a single distance code": 9, "symbol 286": 10, "distance symbol 30": 10, "distance before the block": 11}


def test_the_core_on_the_host_equals_zlib(tmp_path, corpus):
    statuses = _run(_build(tmp_path, False), tmp_path, corpus)
    hand = list(bm.handmade())
    assert dict(zip(hand, statuses[-len(hand):])) == HANDMADE_STATUS
    assert len(set(statuses)) >= 12                                    # the flipped bits reach most refusals as well
    assert 4 * 15 <= statuses.count(-1) <= 4 * 16                     # bits 16 .. 31 of ISIZE in the four blocks (bit 16 of a small ISIZE alone gives 64 KiB + a little)


def test_the_core_under_the_address_and_undefined_sanitizers(tmp_path, corpus):
    """The same corpus through a build of the program with -fsanitize=address,undefined (a program of its own: nothing is preloaded): every block's deflate data and its
    output lie in allocations of exactly their lengths, so a read or write past either stops the program."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined"]
    if subprocess.run(["g++"] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.fail("g++ cannot build and run a program with -fsanitize=address,undefined: the second build of the program is part of this test")
    _run(_build(tmp_path, True), tmp_path, corpus)


def test_file_pieces_gives_bgzf_blocks_compressed_only_when_asked(tmp_path):
    text = fastq(30, 200, 4)
    f = bm.write(text, 700)
    path = tmp_path / "reads.fq.gz"
    path.write_bytes(f)
    host_pieces = list(api.file_pieces(str(path), 3000))
    assert host_pieces == list(api.file_pieces(str(path), 3000, bgzf="host"))
    assert all(type(p) is bytes and fmt == "fastq" for fmt, p, _ in host_pieces) and b"".join(p for _, p, _ in host_pieces) == text
    pieces = list(api.file_pieces(str(path), 3000, bgzf="device"))
    assert all(isinstance(p, api.BgzfPiece) for _, p, _ in pieces) and b"".join(p for _, p, _ in pieces) == f
    assert [last for _, _, last in pieces] == [False] * (len(pieces) - 1) + [True] and len(pieces) > 3
    assert sum(p.text_bytes for _, p, _ in pieces) == len(text)
    for _, p, last in pieces:
        sizes = bm.bgzf_sizes(p)                                          # whole blocks, cut where the ISIZE sum reaches the batch
        assert (last or 3000 <= p.text_bytes < 3000 + 700) and len(sizes) >= 1 and len(gzip.decompress(p)) == p.text_bytes
    with pytest.raises(ValueError):
        list(api.file_pieces(str(path), 3000, bgzf="gpu"))
    # an ordinary member appended: zlib's from there to the end
    path.write_bytes(bm.write(text[:5000], 700, eof=False) + gzip.compress(text[5000:8000]) + bm.write(text[8000:], 700))
    pieces = [p for _, p, _ in api.file_pieces(str(path), 3000, bgzf="device")]
    kinds = [isinstance(p, api.BgzfPiece) for p in pieces]
    assert kinds == sorted(kinds, reverse=True) and any(kinds) and not all(kinds)
    assert b"".join(gzip.decompress(p) if k else p for p, k in zip(pieces, kinds)) == text
    assert sum(len(bm.bgzf_sizes(p)) for p, k in zip(pieces, kinds) if k) == 8
    # a file that does not start with a BGZF block, plain text, and an empty file: as under "host"
    for name, data in (("a.fq.gz", gzip.compress(text[:4000]) + f), ("b.fq", text), ("c.fq.gz", b"")):
        (tmp_path / name).write_bytes(data)
        assert list(api.file_pieces(str(tmp_path / name), 3000, bgzf="device")) == list(api.file_pieces(str(tmp_path / name), 3000))
    # a file cut inside a block ends as a cut gzip file does
    path.write_bytes(f[:len(f) - 40])
    with pytest.raises(EOFError):
        list(api.file_pieces(str(path), 3000, bgzf="device"))


def test_bgzf_member_is_the_headers_definition():
    blk = bm.block(b"hello")
    assert api.bgzf_member(blk) == (len(blk), 5) and api.bgzf_member(b"xx" + blk, 2) == (len(blk), 5)
    assert all(api.bgzf_member(blk[:k]) == 0 for k in range(len(blk)))
    assert api.bgzf_member(gzip.compress(b"hello")) is None and api.bgzf_member(b"\x1f\x8b\x08") == 0 and api.bgzf_member(b"\x1f\x8c") is None
    flg = blk[:3] + b"\x0c" + blk[4:]                                      # FLG must be exactly 4
    assert api.bgzf_member(flg) is None
    other = blk[:10] + b"\x0a\x00XY\x00\x00" + blk[12:]                      # another subfield in front of BC
    other = other[:20] + (len(other) - 1).to_bytes(2, "little") + other[22:]
    assert api.bgzf_member(other) == (len(other), 5) and bm.zlib_verdict(other) == b"hello"
    assert api.bgzf_member(blk[:12] + b"BD" + blk[14:]) is None and api.bgzf_member(blk[:14] + b"\x03" + blk[15:]) is None
    # framed like BGZF but with more than 64 KiB of text: not a BGZF block, so zlib's like any other member
    big = bm.frame(bm.deflate_raw(b"A" * 65537), zlib.crc32(b"A" * 65537), 65537)
    assert bm.zlib_verdict(big) == b"A" * 65537 and api.bgzf_member(big) is None and api.bgzf_member(bm.block(b"A" * 65536))[1] == 65536


def test_big_isize_goes_to_zlib_and_the_refusal_words_are_the_headers(tmp_path):
    text = fastq(90, 400, 6)
    assert len(text) > 70000
    path = tmp_path / "reads.fq.gz"
    path.write_bytes(bm.write(text[:900], 300, eof=False) + bm.frame(bm.deflate_raw(text[900:70000]), zlib.crc32(text[900:70000]), 70000 - 900) + bm.write(text[70000:], 300))
    pieces = [p for _, p, _ in api.file_pieces(str(path), 1 << 20, bgzf="device")]
    assert [isinstance(p, api.BgzfPiece) for p in pieces] == [True] + [False] * (len(pieces) - 1) and bm.bgzf_count(pieces[0]) == 3
    assert b"".join(pieces[1:]) == text[900:]
    header = open(os.path.join(ROOT, "include", "graphchainer_amd.h")).read()
    assert f'#define GC_BGZF_REFUSED "{api.BGZF_REFUSED}"' in header
    assert "GC_BGZF_REFUSED" in open(os.path.join(ROOT, "graphchainer_amd", "csrc", "capi", "gc_capi_reads.hip")).read()
