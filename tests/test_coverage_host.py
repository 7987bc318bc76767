"""The coverage core (csrc/hip/gc_coverage_core.hpp) as an ordinary program (tests/coverage_host/coverage_host_test.cpp), built with g++ once as it is and once with
-fsanitize=address,undefined and run directly. The program runs the kernel's loop over 64 emulated lanes - the predecessor of lane 0 carried from the chunk before, a
ballot of the covering lanes, one of the lanes that open a run of one segment - and the finish step's run marking and line formatting, on the shapes of
coverage_model.shape_sets(): traces of 1, 63, 64, 65 and 129 cells, insertion runs across a chunk boundary, segments of 1, 64, 65 and 130 bp. What it prints is held to
the model's two writers here."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import coverage_model as cm   # noqa: E402

NAMES = ["s1", "", "s3", "a longer name 4"]            # the second segment has no name: it prints as its number, 1


def _hex(b):
    return b.hex() or "-"


def _build(tmp, sanitize):
    exe = str(tmp / ("coverage_host_asan" if sanitize else "coverage_host"))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "graphchainer_amd", "csrc", "hip")] + flags +
                   [os.path.join(ROOT, "tests", "coverage_host", "coverage_host_test.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    return exe


def _run(exe, tmp):
    path = str(tmp / "cases.txt")
    with open(path, "w") as f:
        f.write(f"G {len(NAMES)} " + " ".join(f"{n} {_hex(name.encode())}" for n, name in zip(cm.SHAPE_LENGTHS, NAMES)) + "\n")
        for traces in cm.shape_sets().values():
            for nodes, offsets in traces:
                f.write(f"T {len(nodes)} " + " ".join(f"{a} {b}" for a, b in zip(nodes, offsets)) + "\n")
            f.write("E\n")
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return out.stdout.splitlines()


def _check(lines):
    sets = cm.shape_sets()
    assert len(lines) == 2 * len(sets)
    for k, (name, traces) in enumerate(sets.items()):
        depth = cm.traces_depth(traces)
        assert lines[2 * k] == "S " + _hex(cm.segment_table(NAMES, depth)), name
        assert lines[2 * k + 1] == "B " + _hex(cm.base_table(NAMES, depth)), name


def test_the_shapes_cover_what_they_claim():
    cases = cm.shape_cases()
    assert sorted({len(t[0]) for traces in cases.values() for t in traces} & {1, 63, 64, 65, 129}) == [1, 63, 64, 65, 129]
    nodes, offsets = cases["insertions across the chunk boundary"][0]
    assert len({(nodes[i], offsets[i]) for i in range(59, 69)}) == 1 and offsets[69] == offsets[59] + 1            # cells 60..68 repeat cell 59: lanes 60..63 and 0..4
    depth = cm.traces_depth(cases["129 cells over three segments"])
    assert [int(d.min()) for d in depth[:2]] == [1, 1] and cm.base_table(NAMES, depth).count(b"\n") == 3             # equal depth on both sides of two boundaries, three runs
    everything = cm.traces_depth(cm.shape_sets()["every case"])
    assert {2, 3} <= {int(v) for d in everything for v in d}
    assert int(cm.traces_depth(cases["depth three"])[2][64]) == 3 and int(cm.traces_depth(cases["depth three"])[2][29]) == 0
    both = cm.traces_depth(cases["both strands of s4"])[3]
    assert int(both[19]) == 0 and int(both[20]) == 1 and int(both[46]) == 2 and int(both[109]) == 1 and int(both[110]) == 0
    idle = cm.traces_depth(cm.shape_sets()["s1 stays uncovered"])
    assert int(idle[0].sum()) == 0 and b"s1\t1\t0\n" in cm.segment_table(NAMES, idle) and b"s1\t" not in cm.base_table(NAMES, idle)


def test_lanes_runs_and_lines_on_the_host_equal_the_model(tmp_path):
    _check(_run(_build(tmp_path, False), tmp_path))


def test_lanes_runs_and_lines_under_the_address_and_undefined_sanitizers(tmp_path):
    """The same cases through a build of the program with -fsanitize=address,undefined (a program of its own: nothing is preloaded)."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined"]
    if subprocess.run(["g++"] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 or subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.fail("g++ cannot build and run a program with -fsanitize=address,undefined: the second build of the program is part of this test")
    _check(_run(_build(tmp_path, True), tmp_path))
