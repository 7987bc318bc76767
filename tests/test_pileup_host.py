"""The pileup core (csrc/hip/gc_pileup_core.hpp) as an ordinary program (tests/pileup_host/pileup_host_test.cpp), built with g++ once as it is and once with
-fsanitize=address,undefined and run directly. The program runs the kernel's pileup step over 64 emulated lanes - the predecessor of lane 0, its read position included,
carried from the chunk before - and the finish step's filter and line formatting, on the shapes of pileup_model.shape_sets(): traces of 1, 63, 64, 65 and 129 cells with
reads, mismatches in lanes 0 and 63, insertion and deletion runs across a chunk boundary, both strands, ambiguous graph letters. What it prints is held to the model's
writer here; a cell whose read position lies behind its read is not counted and is reported."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import pileup_model as pm   # noqa: E402

NAMES = ["s1", "", "s3", "a longer name 4"]            # the second segment has no name: it prints as its number, 1
FILTERS = [(0, 0.0), (1, 0.0), (2, 0.0), (0, 0.5), (1, 1.0)]


def _hex(b):
    return b.hex() or "-"


def _build(tmp, sanitize):
    exe = str(tmp / ("pileup_host_asan" if sanitize else "pileup_host"))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "graphchainer_amd", "csrc", "hip")] + flags +
                   [os.path.join(ROOT, "tests", "pileup_host", "pileup_host_test.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    return exe


def _segments():
    return pm.Segments(NAMES, pm.shape_letters())


def _trace_line(item):
    (nodes, offsets), seq_pos, read = item
    return f"T {len(nodes)} {_hex(read)} " + " ".join(f"{a} {b} {c}" for a, b, c in zip(nodes, offsets, seq_pos)) + "\n"


def _run(exe, tmp):
    g = _segments()
    n = sum(g.lengths)
    path = str(tmp / "cases.txt")
    with open(path, "w") as f:
        f.write(f"G {len(NAMES)} " + " ".join(f"{_hex(letters.encode())} {_hex(name.encode())}" for letters, name in zip(g.letters, NAMES)) + "\n")
        for items in pm.shape_sets().values():
            f.write("Z\n")
            for item in items:
                f.write(_trace_line(item))
            for min_alt, fraction in FILTERS:
                f.write(f"E {min_alt} {fraction!r} 0 {n}\n")
            f.write(f"E 1 0.0 0 100\nE 1 0.0 100 {n - 100}\n")
        # a read position behind the read: lane 0 of the second chunk, then the first cell of a trace
        (nodes, offsets), seq_pos, read = pm.shape_cases()["129 cells over three segments"][0]
        f.write("Z\n" + _trace_line(((nodes, offsets), seq_pos[:64] + [len(read)] + seq_pos[65:], read)) + f"E 0 0.0 0 {n}\n")
        f.write("Z\n" + _trace_line((([0], [0]), [1], b"A")) + f"E 0 0.0 0 {n}\n")
        f.write("Z\n" + _trace_line((([0], [0]), [0], b"A")) + f"E 0 0.0 0 {n}\n")
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout.splitlines()


def _check(lines):
    g = _segments()
    n = sum(g.lengths)
    sets = pm.shape_sets()
    per = len(FILTERS) + 2
    assert len(lines) == per * len(sets) + 3
    for k, (name, items) in enumerate(sets.items()):
        p = pm.shape_pileup(items, g)
        got = lines[per * k:per * (k + 1)]
        for (min_alt, fraction), line in zip(FILTERS, got):
            assert line == "P " + _hex(pm.table(p, min_alt=min_alt, min_fraction=fraction)), (name, min_alt, fraction)
        assert got[-2] == "P " + _hex(pm.table(p, 0, 100)) and got[-1] == "P " + _hex(pm.table(p, 100, n - 100)), name
        assert pm.table(p, 0, 100) + pm.table(p, 100, n - 100) == pm.table(p)
    assert lines[-3:-1] == ["BAD", "BAD"]
    assert lines[-1] == "P " + _hex(pm.table(pm.from_cells([0], [0], [0], "A", g), min_alt=0))


def test_lanes_channels_and_lines_on_the_host_equal_the_model(tmp_path):
    _check(_run(_build(tmp_path, False), tmp_path))


def test_lanes_channels_and_lines_under_the_address_and_undefined_sanitizers(tmp_path):
    """The same cases through a build of the program with -fsanitize=address,undefined (a program of its own: nothing is preloaded)."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined"]
    if subprocess.run(["g++"] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.fail("g++ cannot build and run a program with -fsanitize=address,undefined: the second build of the program is part of this test")
    _check(_run(_build(tmp_path, True), tmp_path))
