"""tests/shim_clip/shim_clip_test.cpp: the shim with precise clipping and the X-drop (include/graphchainer_amd_shim.hpp). AlignOneWay accepts the preciseClipping /
preciseClippingIdentityCutoff / Xdropcutoff that match the gc_params_ext gcshim::bind() was given and returns what gc_align_batch_ext returns for it; it refuses others."""
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
    exe = str(tmp_path / "shim_clip_test")
    lib_dir = os.path.join(ROOT, "graphchainer_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "shim_clip", "shim_clip_test.cpp"), "-L" + lib_dir, "-lgraphchainer_amd", "-Wl,-rpath," + lib_dir])
    return exe


def test_shim_clip_driver_builds(tmp_path):
    import graphchainer_amd as gca
    exe = _build(tmp_path)
    if gca.device_count() > 0:
        pytest.skip("a GPU is present: the gpu test runs the program")
    out = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "ref_test_graph.gfa"), "0.66", "5", "ACGT"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "NO_DEVICE", out.stdout + out.stderr


def test_the_shim_no_longer_refuses_the_two_arguments():
    text = open(os.path.join(ROOT, "include", "graphchainer_amd_shim.hpp")).read()
    assert "are not built" not in text
    assert "gc_align_batch_ext" in text


@pytest.mark.gpu
@pytest.mark.parametrize("cutoff,x_drop", [(0.66, 0), (0.9, 5), (0.0, 50), (0.0, 0)])
def test_shim_accepts_the_bound_clipping(tmp_path, cutoff, x_drop):
    import graphchainer_amd as gca
    exe = _build(tmp_path)
    gold = os.path.join(ROOT, "tests", "golden")
    gfa = os.path.join(gold, "syn20k.gfa")
    reads = [l.strip() for l in open(os.path.join(gold, "syn20k.fa")) if not l.startswith(">")][:2]
    rng = random.Random(5)
    reads.append(reads[0][:300] + "".join(rng.choice("ACGT") for _ in range(400)))       # leaves the graph
    out = subprocess.run([exe, gfa, repr(cutoff), str(x_drop)] + reads, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.split("\n")
    refused = [l.split() for l in lines if l.startswith("REFUSED ")]
    assert len(refused) == len(reads) and all(f[2] == f[3] and int(f[3]) >= 2 for f in refused), "the shim accepted values other than the bound ones"
    graph = gca.AlignmentGraph(gfa)
    res = gca.Aligner(graph, gca.MinimizerSeeder(graph), long_pass=True, keep_traces=True, keep_seeds=True, precise_clipping=cutoff, x_drop=x_drop).align_reads([r.encode() for r in reads])
    want = []
    off = np.asarray(res["read_longall_off"], dtype=np.int64)
    toff = np.asarray(res["long_trace_off"], dtype=np.int64)
    for r in range(len(reads)):
        for a in range(off[r], off[r + 1]):
            want.append(f"ALN {r} {int(res['longall_start'][a])} {int(res['longall_end'][a])} {int(res['longall_score'][a])} {int(toff[a + 1] - toff[a])}")
    got = [l for l in lines if l.startswith("ALN ")]
    assert got == want and len(got) >= len(reads)
