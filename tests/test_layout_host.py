"""The device-block layouts of a read batch and a seed batch without a GPU: csrc/host/gc_layout.hpp compiled with g++ into an ordinary program
(tests/layout_host/layout_host_test.cpp) and held to the formulas as gc_reads_upload, the parser and the three seed producers each wrote them out before the layouts were
shared - at the lengths where (len + 63) / 64 + 1, the max(bytes, 1) of an empty part and the 256-byte rounding turn - once as it is and once more built with
-fsanitize=address,undefined."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

READ_CASES = [[], [0], [1], [63], [64], [65], [128, 0, 1], [10000]]
SEED_CASES = [(0, 0), (1, 0), (1, 1), (3, 65)]
ED_READ_BYTES, SEED_HIT_BYTES = 24, 24     # sizeof(EdRead), sizeof(SeedHit)


class Parts:
    """the `part` lambda: the current offset, then on by the bytes (at least 1) rounded up to 256"""
    def __init__(self):
        self.at = 0

    def __call__(self, nbytes):
        here = self.at
        self.at += (max(nbytes, 1) + 255) & ~255
        return here


def reads_want(lens):
    n = len(lens)
    offsets = [0]
    for l in lens:
        offsets.append(offsets[-1] + l)
    out = [n]
    total_words = eq_words = 0
    for r in range(n):
        ln = offsets[r + 1] - offsets[r]
        mask_off, mask_words = total_words, (ln + 63) // 64 + 1
        total_words += 8 * mask_words
        out += [mask_off, mask_words, eq_words, offsets[r], eq_words, ln, mask_words]     # maskOff, maskWords, eqOff, EdRead { readOff, eqOff, len, words }
        eq_words += 4 * mask_words
    total = offsets[n]
    part = Parts()
    out += [total_words, eq_words]
    out += [part(2 * total), part((n + 1) * 8), part(total_words * 8), part(eq_words * 8), part(n * ED_READ_BYTES), part(((total >> 5) + 1) * 8), part(((total >> 6) + 1) * 8),
            part(((total >> 6) + 1) * 4), part(n * 8), part(n * 4), part(n * 8), part(n)]
    return out + [part.at]


def seeds_want(n_reads, n_hits):
    # (the bad-hit part is one 64-bit word in gc_seeds_upload and gc_seeds_mxm and three in gc_seeds_from_store: 256 bytes either way)
    part = Parts()
    one = [part((n_reads + 1) * 4), part(5 * n_hits * 4), part(8), part(n_hits * SEED_HIT_BYTES), part.at]
    part = Parts()
    three = [part((n_reads + 1) * 4), part(5 * n_hits * 4), part(3 * 8), part(n_hits * SEED_HIT_BYTES), part.at]
    assert one == three
    return one


def _build(tmp, sanitize):
    out = str(tmp / ("layout_host_test_san" if sanitize else "layout_host_test"))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "graphchainer_amd", "csrc", "host"),
                    os.path.join(ROOT, "tests", "layout_host", "layout_host_test.cpp"), "-o", out] + flags, check=True, timeout=600)
    return out


def _run(exe, tmp):
    path = str(tmp / "cases.txt")
    with open(path, "w") as f:
        for lens in READ_CASES:
            f.write(" ".join(["reads"] + [str(l) for l in lens]) + "\n")
        for n_reads, n_hits in SEED_CASES:
            f.write(f"seeds {n_reads} {n_hits}\n")
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return [[int(x) for x in line.split()] for line in out.stdout.splitlines()]


def _compare(got):
    want = [reads_want(lens) for lens in READ_CASES] + [seeds_want(*c) for c in SEED_CASES]
    assert len(got) == len(want)
    for g, w, case in zip(got, want, READ_CASES + SEED_CASES):
        assert g == w, case


def test_the_formulas_turn_where_the_cases_say():
    assert [reads_want([l])[2] for l in (0, 1, 63, 64, 65)] == [1, 2, 2, 2, 3]                 # words per bit vector
    assert reads_want([])[-1] == 12 * 256 and seeds_want(0, 0)[-1] == 4 * 256                   # every empty part still takes 256 bytes
    assert seeds_want(3, 65)[1:4] == [256, 256 + 1536, 256 + 1536 + 256]                        # 5 * 65 * 4 = 1300 -> 1536


def test_layout_header_on_the_host_equals_the_formulas(tmp_path):
    _compare(_run(_build(tmp_path, False), tmp_path))


def test_layout_header_under_the_address_and_undefined_sanitizers(tmp_path):
    """The same cases through a build of the program with -fsanitize=address,undefined (a program of its own: nothing is preloaded)."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined"]
    if subprocess.run(["g++"] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.fail("g++ cannot build and run a program with -fsanitize=address,undefined: the second build of the program is part of this test")
    _compare(_run(_build(tmp_path, True), tmp_path))
