"""The FASTA / FASTQ loader without a GPU: csrc/hip/gc_fastx_core.hpp compiled with g++ into an ordinary program (tests/fastx_host/fastx_host_test.cpp) that drives it with
the kernels' tiling - tiles of the newline count, of the scans and of the map composition, and the gather's split of a long line into 16-byte spans - held to
tests/fastx_model.py on the fixtures and on seeded random texts, once as it is and once more built with -fsanitize=address,undefined."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fastx_model as fm                           # noqa: E402
from test_fastx_model import fixture_cases         # noqa: E402


def _cases():
    """(format, final, text): every fixture and every random text, in both formats, final and not."""
    texts = [c[2] for c in fixture_cases()] + fm.random_texts()
    return [(fmt, final, t) for t in texts for fmt in ("fasta", "fastq") for final in (True, False)]


@pytest.fixture(scope="module")
def cases():
    return _cases()


@pytest.fixture(scope="module")
def want(cases):
    return [fm.parse(t, fmt, final) for fmt, final, t in cases]


def _build(tmp, sanitize):
    out = str(tmp / ("fastx_host_test_san" if sanitize else "fastx_host_test"))
    csrc = os.path.join(ROOT, "graphchainer_amd", "csrc")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-I" + os.path.join(csrc, "hip"), os.path.join(ROOT, "tests", "fastx_host", "fastx_host_test.cpp"), "-o", out] + flags,
                   check=True, timeout=600)
    return out


def _run(exe, tmp, cases):
    path = str(tmp / "cases.txt")
    with open(path, "w") as f:
        for fmt, final, text in cases:
            f.write(f"{fmt} {int(final)} {text.hex() or '-'}\n")
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    lines = out.stdout.split("\n")
    got, at = [], 0
    unhex = lambda h: b"" if h == "-" else bytes.fromhex(h)   # noqa: E731
    for _ in cases:
        consumed, n = (int(x) for x in lines[at].split())
        pairs = [l.split(" ") for l in lines[at + 1:at + 1 + n]]
        got.append(([unhex(p[0]) for p in pairs], [unhex(p[1]) for p in pairs], consumed))
        at += 1 + n
    return got


def _compare(got, want, cases):
    assert len(got) == len(want)
    for g, w, (fmt, final, text) in zip(got, want, cases):
        assert g == w, (fmt, final, text[:300])


def test_the_random_texts_reach_every_tile_size_and_both_readers(cases, want):
    assert len(fm.random_texts()) >= 500 + 9 * len(fm.TILE_SIZES) and len(cases) >= 4 * len(fm.random_texts()) >= 2000
    lengths = {len(t) for _, _, t in cases}
    for tile in fm.TILE_SIZES:
        assert {k * tile + d for k in (1, 2, 3) for d in (-1, 0, 1)} <= lengths
    assert set(fm.ALPHABET) <= set(b"".join(t for _, _, t in cases))
    with_reads = sum(1 for w in want if w[0])
    assert with_reads > len(want) // 5
    assert max(len(s) for w in want for s in w[1]) > 4096          # a line longer than a block's gather tile
    assert any(0 < w[2] < len(c[2]) for w, c in zip(want, cases) if not c[1])


def test_core_header_on_the_host_equals_the_model(tmp_path, cases, want):
    _compare(_run(_build(tmp_path, False), tmp_path, cases), want, cases)


def test_core_header_under_the_address_and_undefined_sanitizers(tmp_path, cases, want):
    """The same inputs through a build of the program with -fsanitize=address,undefined (a program of its own: nothing is preloaded): the text lies in an allocation of
    exactly its length, so a read past a line table's or the text's end stops the program."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined"]
    if subprocess.run(["g++"] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.fail("g++ cannot build and run a program with -fsanitize=address,undefined: the second build of the program is part of this test")
    _compare(_run(_build(tmp_path, True), tmp_path, cases), want, cases)
