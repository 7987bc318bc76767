"""The BAM loader's core without a GPU: csrc/hip/gc_bam_core.hpp - the walk over the header and the block_size chain, the per-record checks and the unpacking - built with
g++ into an ordinary program (tests/bam_host/bam_host_test.cpp), once as it is and once more with -fsanitize=address,undefined, and held to tests/bam_model.py's reader on
randomised records from its writer, on every refusal, and on streams cut at every byte with and without FINAL."""
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bam_model as bm                             # noqa: E402

FINAL, HEADER = 1, 2
STATUS = {"magic": 1, "block_size": 2, "name": 3, "l_seq": 4, "span": 5, "cut": 6}   # BamStatus (gc_bam_core.hpp)
ALL = "=ACMGRSVTWYHKDBN"


def _cases():
    rng = random.Random(20)
    cases = []
    for k in range(40):                                                    # whole files: with and without references, every letter
        records = bm.random_records(rng, rng.randrange(0, 12), letters=ALL if k % 2 else "ACGT")
        refs = ((b"chr1", 5), (b"c", 1 << 31), (b"a much longer reference name", 7))[:rng.choice((0, 0, 1, 3))]
        cases.append((FINAL | HEADER, bm.stream(records, text=rng.randbytes(rng.choice((0, 3, 50))), refs=refs)))
    long_read = "".join(rng.choice(ALL) for _ in range(40001))
    cases.append((FINAL | HEADER, bm.stream([(b"a", "ACG", 0), (b"long", long_read, 0x10), (b"b", "T", 4), (b"long2", long_read[:-1], 0x10), (b"n" * 254, long_read[:4097], 0)])))
    cases.append((FINAL, b"".join(bm.record(*r) for r in bm.random_records(rng, 9))))          # a chunk from the middle of a file
    cases += [(FINAL, b""), (0, b""), (HEADER, b""), (FINAL | HEADER, bm.header()), (FINAL | HEADER, bm.header(b"", ()))]
    # every refusal, as the first, a middle and the last record, and behind a record that is left out
    good = [bm.record(*r) for r in bm.random_records(rng, 6, letters=ALL)] + [bm.record(b"x", "ACGT", 0x100)]
    for what in ("block_size", "name", "name0", "l_seq", "span"):
        for at in (0, 3, len(good) - 1):
            recs = list(good)
            recs[at] = bm.damaged(bm.record(b"victim", "ACGTACGTA", 0, (1, 2), b"tag"), what)
            cases.append((FINAL | HEADER, bm.header() + b"".join(recs)))
            cases.append((0, b"".join(recs)))
    two = good[:]
    two[2] = bm.damaged(bm.record(b"v", "ACGT"), "span")
    two[4] = bm.damaged(bm.record(b"v", "ACGT"), "name0")
    cases.append((FINAL, b"".join(two)))                                                    # two refused records: the first one is named
    cases += [(FINAL | HEADER, b"BAM\x02" + bytes(8)), (HEADER, b"BAN\x01" + bytes(8)), (FINAL | HEADER, b"\x1f\x8b\x08\x04" + bytes(20)), (FINAL | HEADER, b"BA"), (HEADER, b"BA")]
    # cut at every byte, FINAL or not, with and without a header
    small = bm.stream([(b"r1", "ACGTA", 0, (5 << 4,), b"xy"), (b"r2", "", 0x800), (b"r3", "GGATC=N", 0x10)], text=b"@CO\tx\n", refs=((b"chr1", 9), (b"chr2", 8)))
    body = small[bm.read_header(small):]
    for cut in range(len(small) + 1):
        cases += [(HEADER, small[:cut]), (FINAL | HEADER, small[:cut])]
    for cut in range(len(body) + 1):
        cases += [(0, body[:cut]), (FINAL, body[:cut])]
    return cases


def _want(flags, raw):
    try:
        ids, reads, skipped, consumed = bm.read_stream(raw, has_header=bool(flags & HEADER), final=bool(flags & FINAL))
    except bm.BamRefused as e:
        return ("ERR", -1 if e.record is None else e.record, e.offset, STATUS[e.why])
    return ("OK", len(ids) + skipped, consumed, skipped, list(zip(ids, reads)))


@pytest.fixture(scope="module")
def cases():
    return _cases()


@pytest.fixture(scope="module")
def want(cases):
    return [_want(flags, raw) for flags, raw in cases]


def _build(tmp, sanitize):
    out = str(tmp / ("bam_host_test_san" if sanitize else "bam_host_test"))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "graphchainer_amd", "csrc", "hip"),
                    os.path.join(ROOT, "tests", "bam_host", "bam_host_test.cpp"), "-o", out] + flags, check=True, timeout=600)
    return out


def _run(exe, tmp, cases):
    path = str(tmp / "cases.txt")
    with open(path, "w") as f:
        for flags, raw in cases:
            f.write(f"{flags} {raw.hex() or '-'}\n")
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.split("\n")
    got, at = [], 0
    for _ in cases:
        head = lines[at].split(" ")
        at += 1
        if head[0] == "ERR":
            got.append(("ERR", int(head[1]), int(head[2]), int(head[3])))
            continue
        n, consumed, skipped = int(head[1]), int(head[2]), int(head[3])
        rows = []
        for row in lines[at:at + n - skipped]:
            name, read = row.split(" ")
            rows.append((b"" if name == "-" else bytes.fromhex(name), "" if read == "-" else read))
        at += n - skipped
        got.append(("OK", n, consumed, skipped, rows))
    assert lines[at:] == [""]
    return got


def _compare(got, want, cases):
    assert len(got) == len(want)
    for k, (g, w, (flags, raw)) in enumerate(zip(got, want, cases)):
        assert g == w, (k, flags, len(raw), raw[:120].hex(), g[:4], w[:4])


def test_the_cases_cover_what_they_claim(cases, want):
    assert {w[3] for w in want if w[0] == "ERR"} == set(STATUS.values())
    assert {w[1] for w in want if w[0] == "ERR"} >= {-1, 0, 3, 6}
    good = [w for w in want if w[0] == "OK"]
    assert any(w[3] for w in good) and any(w[1] == 0 and w[2] > 0 for w in good) and any(w[2] == 0 for w in good)
    reads = [read for w in good for _, read in w[4]]
    assert {len(r) for r in reads} >= {0, 1, 2, 15, 16, 17, 31, 32, 33, 4097, 40000, 40001} and set("".join(reads)) == set(ALL)
    assert {len(name) for w in good for name, _ in w[4]} >= {1, 254}
    assert any(0 < w[2] < len(raw) for w, (flags, raw) in zip(want, cases) if w[0] == "OK" and not flags & FINAL)   # a chunk that ends inside a record


def test_walk_fields_and_unpack_on_the_host_equal_the_model(tmp_path, cases, want):
    _compare(_run(_build(tmp_path, False), tmp_path, cases), want, cases)


def test_walk_fields_and_unpack_under_the_address_and_undefined_sanitizers(tmp_path, cases, want):
    """The same inputs through a build of the program with -fsanitize=address,undefined (a program of its own: nothing is preloaded): every case's bytes lie in an
    allocation of exactly their length, so a read past their end stops the program."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined"]
    if subprocess.run(["g++"] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.fail("g++ cannot build and run a program with -fsanitize=address,undefined: the second build of the program is part of this test")
    _compare(_run(_build(tmp_path, True), tmp_path, cases), want, cases)
