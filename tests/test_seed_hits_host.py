"""Caller-supplied seed hits, the parts that need no GPU: the per-hit functions of csrc/hip/gc_seedhits_core.hpp compiled with g++ (tests/seedhits_host/seedhits_host_test.cpp),
and the order of the entry points' checks on a machine without a device."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("seedhits") / "seedhits_host_test")
    csrc = os.path.join(ROOT, "graphchainer_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(csrc, "host"), "-I" + os.path.join(csrc, "hip"), os.path.join(ROOT, "tests", "seedhits_host", "seedhits_host_test.cpp"),
                    os.path.join(csrc, "host", "gc_graph.cpp"), "-o", out, "-lpthread", "-lz"], check=True, timeout=600)
    return out


@pytest.mark.parametrize("gfa,short", [("syn20k.gfa", ["short"]), ("ref_test_graph.gfa", [])])
def test_resolve_equals_get_unitig_node_and_the_window_rule_equals_the_two_pointers(exe, gfa, short):
    """Over every (bigraph id, offset) of the graph seedHitResolve gives GetUnitigNode's split node and the offset in it, and refuses what lies outside; over random seed lists with
    matchLen 2..100, duplicates and up to 200 seeds (more than one 64-lane turn of the running maximum) seedWindow gives the windows of the literal loop of src/Aligner.cpp:672-679."""
    out = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", gfa)] + short, capture_output=True, text=True, timeout=600)   # (short: syn20k has segments that end in a short split node)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr


def test_malformed_calls_are_refused_before_a_device_is_needed():
    """The entry points check their arguments on the host first: without a GPU a malformed call is GC_ERR_INVALID (-1), never GC_ERR_DEVICE (-3). A graph or a read batch cannot be
    made without a device, so the calls a machine without one can make are the ones with a null handle; with real handles the same order - offsets and counts before the device,
    the resolve kernel's bounds after it - is what tests/test_seed_hits_gpu.py runs."""
    import graphchainer_amd as gca
    if not os.path.exists(gca.api.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = gca.load_library()
    off = (C.c_uint64 * 2)(0, 0)
    handle, res = C.c_void_p(), C.c_void_p()
    params = gca.api.GcParams()
    lib.gc_params_default(C.byref(params))
    assert lib.gc_seeds_upload(None, None, None, off, 1, C.byref(handle)) == -1 and b"null" in lib.gc_last_error()
    assert lib.gc_seeds_upload(None, None, None, None, 0, None) == -1
    lib.gc_align_batch_seeded.argtypes = [C.c_void_p] * 6
    assert lib.gc_align_batch_seeded(None, None, None, None, C.byref(params), C.byref(res)) == -1 and b"null" in lib.gc_last_error()
    assert not handle.value and not res.value
    lib.gc_seeds_destroy(None)
    assert {"gc_seeds_upload", "gc_seeds_destroy", "gc_align_batch_seeded"} <= set(gca.api.EXPORTED_SYMBOLS)
    if gca.device_count() == 0:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            gca.AlignmentGraph(os.path.join(ROOT, "tests", "golden", "syn20k.gfa"))
