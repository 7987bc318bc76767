"""tests/shim_global/shim_global_test.cpp: the shim with the forced global alignment (include/graphchainer_amd_shim.hpp). AlignOneWay accepts the forceGlobal
that gcshim::bind() was given and returns what gc_align_batch returns for it; it refuses the other value."""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "shim_global_test")
    lib_dir = os.path.join(ROOT, "graphchainer_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "shim_global", "shim_global_test.cpp"), "-L" + lib_dir, "-lgraphchainer_amd", "-Wl,-rpath," + lib_dir])
    return exe


def test_shim_global_driver_builds(tmp_path):
    import graphchainer_amd as gca
    exe = _build(tmp_path)
    if gca.device_count() > 0:
        pytest.skip("a GPU is present: the gpu test runs the program")
    out = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "ref_test_graph.gfa"), "1", "ACGT"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "NO_DEVICE", out.stdout + out.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("force", [1, 0])
def test_shim_accepts_the_bound_forced_global_alignment(tmp_path, force):
    import graphchainer_amd as gca
    exe = _build(tmp_path)
    gold = os.path.join(ROOT, "tests", "golden")
    gfa = os.path.join(gold, "syn20k.gfa")
    reads = [l.strip() for l in open(os.path.join(gold, "syn20k.fa")) if not l.startswith(">")][:2]
    rng = random.Random(5)
    reads.append(reads[0][:300] + "".join(rng.choice("ACGT") for _ in range(400)))       # leaves the graph: the default clips it, the forced run does not
    out = subprocess.run([exe, gfa, str(force)] + reads, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.split("\n")
    refused = [l.split() for l in lines if l.startswith("REFUSED ")]
    assert [int(f[2]) for f in refused] == [1] * len(reads), "the shim accepted a forceGlobal other than the bound one"
    graph = gca.AlignmentGraph(gfa)
    res = gca.Aligner(graph, gca.MinimizerSeeder(graph), long_pass=True, keep_traces=True, keep_seeds=True, force_global=bool(force)).align_reads([r.encode() for r in reads])
    want = []
    off = np.asarray(res["read_longall_off"], dtype=np.int64)
    toff = np.asarray(res["long_trace_off"], dtype=np.int64)
    for r in range(len(reads)):
        for a in range(off[r], off[r + 1]):
            want.append(f"ALN {r} {int(res['longall_start'][a])} {int(res['longall_end'][a])} {int(res['longall_score'][a])} {int(toff[a + 1] - toff[a])}")
    got = [l for l in lines if l.startswith("ALN ")]
    assert got == want and len(got) >= len(reads)
    ends = [int(l.split()[3]) for l in got if l.split()[1] == "2"]
    assert (max(ends) == len(reads[2])) == bool(force)
