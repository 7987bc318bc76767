"""tests/shim_graphaligner/shim_graphaligner_test.cpp: the shim with --seeds-extend-density / --extra-heuristic bound (include/graphchainer_amd_shim.hpp). The whole-read
AlignOneWay accepts the bound values and returns what gc_align_batch returns for them; it refuses another density or the other flag, and the fragment call refuses a density."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "shim_graphaligner_test")
    lib_dir = os.path.join(ROOT, "graphchainer_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "shim_graphaligner", "shim_graphaligner_test.cpp"), "-L" + lib_dir, "-lgraphchainer_amd", "-Wl,-rpath," + lib_dir])
    return exe


def test_shim_graphaligner_driver_builds_and_starts(tmp_path):
    """Without a device the library refuses to create the graph and the program says so; with one it runs a tiny read through."""
    exe = _build(tmp_path)
    out = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "ref_test_graph.gfa"), "-1", "0", "ACGT"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "NO_DEVICE" or "REFUSED 0 1 1 1 1 ACCEPTED 1" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("density,flag", [(-1.0, 0), (-1.0, 1), (0.0005, 0), (0.0005, 1)])
def test_shim_accepts_the_bound_heuristics_and_nothing_else(tmp_path, density, flag):
    import graphchainer_amd as gca
    from graphchainer_amd.synth import SynthGraph
    exe = _build(tmp_path)
    sg = SynthGraph(40_000, seed=23, repeats=3)
    gfa = str(tmp_path / "g.gfa")
    sg.write_gfa(gfa)
    bb = sg.backbone.tobytes().decode()
    reads = [bb[4000:4500] + bb[20000:20500], bb[7000:7400] + bb[25000:25450], bb[15000:15064]]
    out = subprocess.run([exe, gfa, repr(density), str(flag)] + reads, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.split("\n")
    assert [l for l in lines if l.startswith("REFUSED ")] == [f"REFUSED {r} 1 1 1 1 ACCEPTED 1" for r in range(len(reads))]
    graph = gca.AlignmentGraph(gfa)
    res = gca.Aligner(graph, gca.MinimizerSeeder(graph), long_pass=True, keep_traces=True, keep_seeds=True, seed_extend_density=density, extra_heuristic=bool(flag),
                      colinear_chaining=density == -1).align_reads([r.encode() for r in reads])
    off = np.asarray(res["read_longall_off"], dtype=np.int64)
    toff = np.asarray(res["long_trace_off"], dtype=np.int64)
    want = []
    for r in range(len(reads)):
        for a in range(off[r], off[r + 1]):
            want.append(f"ALN {r} {int(res['longall_start'][a])} {int(res['longall_end'][a])} {int(res['longall_score'][a])} {int(toff[a + 1] - toff[a])}")
    assert [l for l in lines if l.startswith("ALN ")] == want and len(want) >= len(reads)
    assert [l for l in lines if l.startswith("EXTENDED ")] == [f"EXTENDED {r} {int(res['seeds_extended_long'][r])}" for r in range(len(reads))]
    assert (len(want) == len(reads)) == (density != -1)          # a budget of one seed: the chimeras keep one alignment
